/* xnwan_eval_grad.h -- extension of the C ABI of libxnwan.so (include/xnwan.h, xnwan_eval.h and xnwan_grad.h, which stay as they
 * are): the gradient and the time derivative of u at scattered space-time points with solver 'dopri5' -- the per-path forward of
 * xnwan_eval.h with its checkpoints kept (csrc/xw_tdopri_paths.hip: the same kernel, one more output) and the reverse sweep over
 * every path's own record (csrc/xw_tdopri_paths_grad.hip).  Conventions as in xnwan.h: device pointers owned by the caller,
 * `stream` a hipStream_t, 0 = ok / negative XW_E_* / positive hipError_t.
 *
 * THE CHECKPOINTING FORWARD.  xw_paths_dopri5_ckpt_fwd is xw_paths_dopri5_fwd (xnwan_eval.h: every word there holds) on jobs that
 * carry one more optional output:
 *   ckpt : NULL, or ckpt[cap][H][N] with the job's f.cap >= 1: slot s of path p holds the state y at the START of p's accepted step
 *          s.  Slot 0 is the lifted start value: always written, also for a path with t_end == t_in.  Slots 1 .. min(n_acc[p], cap) - 1
 *          are written at their accepts; nothing else is touched (not slot n_acc[p], the state behind the last step).
 * u, Y, rec, n_acc, n_att, status and fin are the same bits with and without ckpt; f.cap counts the slots of rec and of ckpt.
 * Refused on the host as xw_paths_dopri5_fwd refuses, and XW_E_ARG for a ckpt with cap < 1.
 *
 * THE SWEEP.  A job is a job of the checkpointing forward after that pass, every path ended with status 0: path p has xT[.][p]
 * ([d][N]), start[p], t_in[p], t_end[p], its count n_acc[p] <= cap, its accepted steps rec[cap][2][N] (t0 and dt) and the states
 * ckpt[cap][H][N] at their starts; Y[H][N] is the forward's y(t_end), needed for ut only.  Slots of rec and ckpt at or past
 * n_acc[p] are never read.  With u_p = FL(y_p(t_end)), the forward's value:
 *   gx[d][N] : du_p/dx_p with the start value and the path's recorded steps held fixed
 *   gs[N]    : du_p/dstart_p
 *              -- both the DISCRETE adjoint: the exact reverse of the accepted steps, step sizes as constants (xw_tdopri5_sweep's
 *              convention); what autograd gives through the restated dopri5 on the one-path group with the sample times
 *              [t_in, t_end] and the controller replaced by the recorded (t0, dt).  The last accepted step (t0 < t_end <= t1)
 *              enters through its quartic dense output y_s + dt sum_j w_j(x) k_j, x = (t_end - t0) / (t1 - t0): the stage
 *              cotangents are dt w_j(x) FL_w, FL_w goes onto y_s, nothing arrives through y_{s+1}; earlier steps have
 *              dt b_j lam, and the cotangent of k_0 of step s + 1 carried into k_6 (FSAL: that field value is taken once, only
 *              step 0 takes its own).  A path without a step has gx = 0 exactly and gs from the lift alone.
 *   ut[N]    : FL_w . F(t_end, x_p, Y_p) at the path's end time and final state -- the time derivative of the CONTINUOUS model
 *              y' = F, u = FL y at fixed x.  It is NOT the derivative of the discrete u with respect to the end time of its grid:
 *              that would need d(step)/d(dt), which nothing here builds.
 * gx, gs and ut may each be NULL, not all three.  One wave per 16-path tile walks s = S - 1 .. 0, S the largest count among its
 * paths (counts are clamped to 0 .. cap); every lane carries its own path's count, t0 and dt; a lane whose path has n_acc <= s takes
 * dt = 0 and the state of its last own slot, which makes the round the exact identity for it -- a path's bits do not depend on the
 * paths beside it.  No float atomics, no waits between tiles, no host read-back: the launch can be captured.
 * work: xw_paths_dopri5_grad_work(d, H, K, m) doubles per 16-path tile -- the tiled dopri5 sweep's, xw_tdopri5_work(1, ...) --
 * times the launch's tiles, the sum over the jobs of (N + 15) / 16, in job order.
 * Refused on the host before any launch: XW_E_ARG for null pointers (jobs, theta, work, a job's xT, start, t_in, t_end, n_acc, rec,
 * ckpt; gx, gs and ut all null; ut without Y), njobs < 1, N < 1, cap < 1; XW_E_DIMS where xw_tiled_ode_ok(d, H, K, m) is 0. */
#ifndef XNWAN_EVAL_GRAD_H
#define XNWAN_EVAL_GRAD_H
#include "xnwan_eval.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct { XwPathsDopriJob f; double* ckpt; } XwPathsDopriCkptJob;
int xw_paths_dopri5_ckpt_fwd(const XwPathsDopriCkptJob* jobs, int njobs, const double* theta, int d, int H, int K, int m, int Hn,
                             double rtol, double atol, int max_steps, int max_attempts, double* work, void* stream);

typedef struct { const double* xT; const double* start; const double* t_in; const double* t_end; const int* n_acc;
                 const double* rec; const double* ckpt; const double* Y; double* gx; double* gs; double* ut; int N;
                 int cap; } XwPathsDopriGradJob;
int xw_paths_dopri5_grad_work(int d, int H, int K, int m);   /* doubles per 16-path tile == xw_tdopri5_work(1, ...) */
int xw_paths_dopri5_grad(const XwPathsDopriGradJob* jobs, int njobs, const double* theta, int d, int H, int K, int m,
                         double* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
