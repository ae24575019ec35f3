/* xnwan_jet.h -- extension of the C ABI of libxnwan.so (include/xnwan.h, xnwan_eval.h, xnwan_grad.h, xnwan_eval_grad.h and
 * xnwan_hess.h, which stay as they are): quadratic forms of the Hessian of u at scattered space-time points, a second-order FORWARD
 * jet over a RAGGED group with a time grid per path (csrc/xw_tiled_paths_jet.hip).  Conventions as in xnwan.h: device pointers owned
 * by the caller, `stream` a hipStream_t, 0 = ok / negative XW_E_* / positive hipError_t.
 *
 * A job is a job of xw_paths_tiled_fwd (xnwan.h) -- path p has the spatial point xT[.][p] ([d][N]), the start value start[p], its own
 * non-decreasing times tT[l][p], l < L ([L][N]; a shorter path repeats its last time) and nstep[N] (may be NULL), the index of its
 * last distinct time -- with R DIRECTIONS per path and NO checkpoints: vx[R][d][N], vs[R][N] and qs[R][N] (may be NULL: zeros).
 * With U_p(x, s) = FL(y_{n_p}), the DISCRETE solution of path p as a function of its point and its start value, grid and step sizes
 * held fixed (method 0 euler, 1 midpoint, 2 rk4 by the 3/8 rule), and the curve
 *   gamma_r(eps) = (x + eps vx_r, s + eps vs_r + eps^2 / 2 qs_r):
 *   u[N]        : U_p itself, the bits of xw_paths_tiled_fwd (may be NULL)
 *   ju[R][N]    : d/deps U(gamma_r) at 0     = dU/dx . vx_r + dU/ds vs_r
 *   quu[R][N]   : d^2/deps^2 U(gamma_r) at 0 = (vx_r, vs_r)^T Hess U (vx_r, vs_r) + dU/ds qs_r
 * ju and quu may each be NULL, not both.  The lift and the hidden layers of the field are ReLU; their kinks are treated as autograd
 * treats them, the gates are constants.  Time is not perturbed.
 * One wave per block, grid (tiles, R): a block recomputes the primal trajectory of its 16 paths from `start` (no checkpoint is read)
 * and carries the jet (y, y', y'') of its direction behind every stage; the blocks of direction 0 store u.  A zero-length step is
 * the exact identity of all three orders, so a path's bits depend neither on the paths beside it nor on the hint, nor on the other
 * directions of the launch; a path without a step has ju = dU/ds vs and quu = dU/ds qs, and quu = 0 exactly where qs = 0.
 * One launch per job on `stream`.  No LDS, no float atomics, no waits between blocks, no host read-back: the launch can be captured.
 * work: xw_paths_tiled_jet_work(d, H, K, m) doubles per BLOCK -- -1 where xw_tiled_ode_ok(d, H, K, m) is 0 -- times the launch's
 * blocks, the sum over the jobs of R (N + 15) / 16, in job order; within a job the block of (tile, direction r) is tile + tiles r.
 * Refused on the host before any launch: XW_E_ARG for null pointers (jobs, theta, work, a job's xT, start, tT, vx, vs; ju and quu
 * both null), njobs < 1, N < 1, R < 1 or R > 65535 (the grid's second dimension), L < 1, a method outside 0..2; XW_E_DIMS where xw_tiled_ode_ok(d, H, K, m) is 0. */
#ifndef XNWAN_JET_H
#define XNWAN_JET_H
#include "xnwan.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct { const double* xT; const double* start; const double* tT; const int* nstep; const double* vx; const double* vs;
                 const double* qs; double* u; double* ju; double* quu; int N; int R; } XwPathsJetJob;
int xw_paths_tiled_jet_work(int d, int H, int K, int m);   /* doubles per block (tile, direction), or -1 */
int xw_paths_tiled_jet(const XwPathsJetJob* jobs, int njobs, const double* theta, int method, int L,
                       int d, int H, int K, int m, double* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
