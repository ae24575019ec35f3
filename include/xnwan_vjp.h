/* xnwan_vjp.h -- extension of the C ABI of libxnwan.so (include/xnwan.h, which stays as it is): PARAMETER gradients of u at
 * scattered space-time points, a reverse sweep over a RAGGED group with a time grid per path that writes slabs
 * (csrc/xw_tiled_paths_vjp.hip).  Conventions as in xnwan.h: device pointers owned by the caller, `stream` a hipStream_t,
 * 0 = ok / negative XW_E_* / positive hipError_t.
 *
 * A job is a job of xw_paths_tiled_grad (xnwan_grad.h) with a weight per path: path p has the spatial point xT[.][p] ([d][N]), the
 * start value start[p], its own non-decreasing times tT[l][p], l < L ([L][N]; a shorter path repeats its last time), the checkpoints
 * Y[L][H][N] that xw_paths_tiled_fwd wrote (NOT last_only) and the weight w[p]; nstep[N] (may be NULL) is the forward's hint, the
 * index of each path's last distinct time.  The forward is never recomputed.
 *
 * What is differentiated: u_p = U_p(theta) = FL(y_{n_p}), the DISCRETE final value of path p -- the exact reverse of the steps taken
 * (method 0 euler, 1 midpoint, 2 rk4 by the 3/8 rule) with the path's grid and step sizes held fixed, its start value start[p] a
 * constant of theta, and the ReLU gates constants as autograd takes them: what autograd through the reference's fixed-grid odeint
 * gives for sum_p w_p u_p, every path taken alone.
 *   gslab[(N + 15) / 16][P_u] : row k is the share of the 16-path tile k of g = sum_p w_p dU_p/dtheta, P_u = the size of theta (the
 *              generic layout at (d, H, K)) and its order -- the slab format of xw_tiled_ode_bwd, xw_tiled_ode_bwd_slabs(N) rows;
 *              xw_slab_sum over the rows gives g.  The entry point zeroes it on the stream before the launch; every entry is then
 *              updated by one fixed lane in program order, so the same launch twice gives the same bits.  A parameter the network
 *              does not use (the hidden layers' slot at m = 1) keeps exact zeros.
 *   gx[d][N] : w_p dU_p/dx_p with the start value and the grid held fixed (may be NULL)
 *   gs[N]    : w_p dU_p/dstart_p (may be NULL)
 * One wave per 16-path tile walks min(L - 1, max nstep over the tile) steps back from the cotangent w_p on every path's final value.
 * A zero-length step is the exact identity of the reverse, a path with w_p = 0 leaves every slab entry's bits as they are, and the
 * lanes of a tile past the end of a job carry the weight 0: they add exact zeros.  No float atomics, no waits between tiles, no host
 * read-back: the launch can be captured.
 * work: xw_paths_tiled_vjp_work(d, H, K, m) doubles per 16-path tile -- at least xw_paths_tiled_grad_work's; -1 where
 * xw_tiled_ode_ok(d, H, K, m) is 0 -- times the launch's tiles, the sum over the jobs of (N + 15) / 16, in job order.
 * Refused on the host before any launch: XW_E_ARG for null pointers (jobs, theta, work, a job's xT, start, tT, Y, w, gslab),
 * njobs < 1, N < 1, L < 1, a method outside 0..2; XW_E_DIMS where xw_tiled_ode_ok(d, H, K, m) is 0. */
#ifndef XNWAN_VJP_H
#define XNWAN_VJP_H
#include "xnwan.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct { const double* xT; const double* start; const double* tT; const int* nstep;
                 const double* Y; const double* w; double* gslab; double* gx; double* gs; int N; } XwPathsVjpJob;
int xw_paths_tiled_vjp_work(int d, int H, int K, int m);   /* doubles per 16-path tile, or -1 */
int xw_paths_tiled_vjp(const XwPathsVjpJob* jobs, int njobs, const double* theta, int method, int L,
                       int d, int H, int K, int m, double* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
