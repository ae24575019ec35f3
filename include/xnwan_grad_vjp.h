/* xnwan_grad_vjp.h -- extension of the C ABI of libxnwan.so (include/xnwan.h, xnwan_hess.h and xnwan_vjp.h, which stay as they
 * are): PARAMETER gradients of u, of its gradient in x along a direction and of its time derivative at scattered space-time points
 * -- the tangent of xw_paths_tiled_vjp's slab-writing sweep along a direction per path, with one term at the top of the sweep for
 * the time derivative (csrc/xw_tiled_paths_gvjp.hip).  Conventions as in xnwan.h: device pointers owned by the caller, `stream` a
 * hipStream_t, 0 = ok / negative XW_E_* / positive hipError_t.
 *
 * A job is a job of xw_paths_tiled_hvp (xnwan_hess.h) whose tangent forward has RUN: path p has the spatial point xT[.][p] ([d][N]),
 * the start value start[p], its own non-decreasing times tT[l][p], l < L ([L][N]; a shorter path repeats its last time), the
 * checkpoints Y[L][H][N] that xw_paths_tiled_fwd wrote (NOT last_only), nstep[N] (may be NULL), the forward's hint, the direction
 * vx[d][N], vs[N] and the tangent checkpoints Yd[L][H][N] along that direction.  Yd is READ here, not written: the caller runs
 * xw_paths_tiled_hvp on the same job with ju alone first, which launches the tangent forward only.  Neither forward is recomputed.
 * Besides the direction a path has two weights, wu[p] and wt[p].
 *
 * What is differentiated, with U_p(theta; x, s) = FL(y_{n_p}) the DISCRETE final value of path p as xnwan_vjp.h defines it -- the
 * exact reverse of the steps taken (method 0 euler, 1 midpoint, 2 rk4 by the 3/8 rule), the path's grid and step sizes held fixed,
 * its start value and the direction constants of theta, the ReLU gates constants as autograd takes them --:
 *   J = sum_p [ wu_p U_p + (dU_p/dx . vx_p + dU_p/ds vs_p) + wt_p ut_p ],   ut_p = FL_w . F(t_p, x_p, y_{n_p}),
 * the middle term xw_paths_tiled_hvp's ju and ut_p xw_paths_tiled_grad's ut: the time derivative of the CONTINUOUS model at the
 * path's end, theta entering through FL_w, through the field's own parameters and through y_{n_p}.  Time is not perturbed.
 *   gslab[(N + 15) / 16][P_u] : row k is the share of the 16-path tile k of dJ/dtheta, P_u = the size of theta (the generic layout at
 *              (d, H, K)) and its order -- the slab format of xw_tiled_ode_bwd; xw_slab_sum over the rows gives dJ/dtheta.  The entry
 *              point zeroes it on the stream before the launch; every entry is then updated by one fixed lane in program order, so
 *              the same launch twice gives the same bits.  A parameter the network does not use (the hidden layers' slot at m = 1)
 *              keeps exact zeros.
 * wu and wt may each be NULL: zeros.  vx and vs may be NULL TOGETHER: no direction, and Yd is not read (it may be NULL then).  At
 * least one of wu, wt, vx must be given.  J is linear in (wu, wt, vx, vs): a path whose weights and direction are zero leaves every
 * slab entry's bits as they are, the lanes of a tile past the end of a job carry exact zeros, and a zero-length step is the exact
 * identity of the sweep.  One wave per 16-path tile, one launch per job; no float atomics, no LDS, no waits between tiles, no host
 * read-back: the launch can be captured.
 * work: xw_paths_tiled_gvjp_work(d, H, K, m) doubles per 16-path tile -- this entry's own size: xw_paths_tiled_hvp_work's, the
 * stage times and weights of the 16 paths and a tangent per layer of the field; -1 where xw_tiled_ode_ok(d, H, K, m) is 0 -- times
 * the launch's tiles, the sum over the jobs of (N + 15) / 16, in job order.
 * Refused on the host before any launch: XW_E_ARG for null pointers (jobs, theta, work, a job's xT, start, tT, Y, gslab; one of vx
 * and vs without the other; vx without Yd; wu, wt and vx all null), njobs < 1, N < 1, L < 1, a method outside 0..2; XW_E_DIMS where
 * xw_tiled_ode_ok(d, H, K, m) is 0. */
#ifndef XNWAN_GRAD_VJP_H
#define XNWAN_GRAD_VJP_H
#include "xnwan_hess.h"
#include "xnwan_vjp.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct { const double* xT; const double* start; const double* tT; const int* nstep; const double* Y; const double* Yd;
                 const double* vx; const double* vs; const double* wu; const double* wt; double* gslab; int N; } XwPathsGvjpJob;
int xw_paths_tiled_gvjp_work(int d, int H, int K, int m);   /* doubles per 16-path tile, or -1 */
int xw_paths_tiled_gvjp(const XwPathsGvjpJob* jobs, int njobs, const double* theta, int method, int L,
                        int d, int H, int K, int m, double* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
