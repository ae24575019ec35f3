/* xnwan_hess.h -- extension of the C ABI of libxnwan.so (include/xnwan.h, xnwan_eval.h, xnwan_grad.h and xnwan_eval_grad.h, which
 * stay as they are): second derivatives of u at scattered space-time points, a Hessian-vector product over a RAGGED group with a
 * time grid per path (csrc/xw_tiled_paths_hvp.hip).  Conventions as in xnwan.h: device pointers owned by the caller, `stream` a
 * hipStream_t, 0 = ok / negative XW_E_* / positive hipError_t.
 *
 * A job is a job of xw_paths_tiled_grad (xnwan_grad.h) -- path p has the spatial point xT[.][p] ([d][N]), the start value start[p],
 * its own non-decreasing times tT[l][p], l < L ([L][N]; a shorter path repeats its last time), the checkpoints Y[L][H][N] that
 * xw_paths_tiled_fwd wrote (NOT last_only) and nstep[N] (may be NULL), the forward's hint -- with a DIRECTION per path:
 * vx[d][N] and vs[N].  With U_p(x, s) = FL(y_{n_p}), the DISCRETE solution of path p as a function of its point and its start
 * value, grid and step sizes held fixed (method 0 euler, 1 midpoint, 2 rk4 by the 3/8 rule):
 *   ju[N]        : dU_p/dx . vx_p + dU_p/ds vs_p, the directional derivative
 *   hx[d][N],
 *   hs[N]        : the (d + 1)-dimensional Hessian of U_p in (x, s) applied to (vx_p, vs_p): the derivative of xw_paths_tiled_grad's
 *                  (gx, gs) along the direction.  The lift and the hidden layers of the field are ReLU; their kinks are treated as
 *                  autograd treats them, the gates are constants.  What autograd's double backward gives for the one-path job.
 *   Yd[L][H][N]  : the tangent checkpoints, row l the derivative of y_l along the direction, so that Yd[0] = d lift(s)/ds vs; the
 *                  rows behind a path's last step repeat its final tangent, as Y's repeat its final state.  Scratch of the job
 *                  that the caller allocates: required, every element is written, and the contents are defined as above.
 * Time is not perturbed: no second derivative in t or mixed in (t, x), and xw_paths_tiled_grad's ut is not differentiated.
 * ju, hx and hs may each be NULL, not all three.  One wave per 16-path tile; two launches per job on `stream`: a tangent forward
 * over Y (it recomputes the stages inside a step, never the trajectory; it writes Yd and ju) and, when hx or hs is asked for, a
 * reverse sweep over Y and Yd.  A zero-length step is the exact identity of both, so a path's bits depend neither on the paths
 * beside it nor on the hint, and a path without a step has hx = 0 and hs = 0 exactly and ju = gs vs.  No float atomics, no waits
 * between tiles, no host read-back: the launches can be captured.
 * work: xw_paths_tiled_hvp_work(d, H, K, m) doubles per 16-path tile -- this entry's own size, larger than the gradient sweep's;
 * -1 where xw_tiled_ode_ok(d, H, K, m) is 0 -- times the launch's tiles, the sum over the jobs of (N + 15) / 16, in job order.
 * Refused on the host before any launch: XW_E_ARG for null pointers (jobs, theta, work, a job's xT, start, tT, Y, vx, vs, Yd; ju,
 * hx and hs all null), njobs < 1, N < 1, L < 1, a method outside 0..2; XW_E_DIMS where xw_tiled_ode_ok(d, H, K, m) is 0. */
#ifndef XNWAN_HESS_H
#define XNWAN_HESS_H
#include "xnwan.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct { const double* xT; const double* start; const double* tT; const int* nstep; const double* Y;
                 const double* vx; const double* vs; double* Yd; double* ju; double* hx; double* hs; int N; } XwPathsHvpJob;
int xw_paths_tiled_hvp_work(int d, int H, int K, int m);   /* doubles per 16-path tile, or -1 */
int xw_paths_tiled_hvp(const XwPathsHvpJob* jobs, int njobs, const double* theta, int method, int L,
                       int d, int H, int K, int m, double* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
