/* xnwan_eval.h -- extension of the C ABI of libxnwan.so (include/xnwan.h, which stays as it is): solver 'dopri5' at scattered
 * space-time points, a step controller PER PATH (csrc/xw_tdopri_paths.hip).  Conventions as in xnwan.h: device pointers owned by
 * the caller, `stream` a hipStream_t, 0 = ok / negative XW_E_* / positive hipError_t.
 *
 * Path p of a job has the spatial point xT[.][p] ([d][N]), the start value start[p], the entry time t_in[p] and the end time
 * t_end[p] >= t_in[p].  u[p] is what the reference's odeint gives for the ONE-PATH group (x_p, start_p) with the sample times
 * [t_in[p], t_end[p]] and no options -- torchdiffeq's dopri5 as xnwan.h states it for xw_dopri5_*: the lift, f0, both halves of
 * _select_initial_step, attempts with accept / reject and the next step size, FSAL, the quartic dense output at t_end from the
 * accepted step with t0 < t_end <= t1 (steps are never clipped), the read-out -- with the RMS norms over that path's Hn entries
 * alone (Hn = the network's u_hidden_dim <= H; zero padding adds exact zeros).  The whole integration of a 16-path tile is ONE
 * launch of one wave, the field on v_mfma_f64_16x16x4; t0, dt, the counts, the done flag and the status live per lane.  A path that
 * is done walks along with dt = 0 and commits nothing; a tile ends when all its paths are done or after max_attempts rounds -- a
 * hard bound inside the kernel, which torchdiffeq does not have (its loop is bounded by max_num_steps accepted steps only).
 * No float atomics, no tickets, no waits between tiles, no host read-back: a path's bits do not depend on the paths beside it, and
 * the launch can be captured.
 *   u[N]        : FL(y(t_end)); t_end == t_in takes no step and gives the read-out of y0.  For a path whose status is not 0 it
 *                 is the read-out of y0 (written, not meaningful)
 *   status[N]   : 0, or XW_DOPRI_UNDERFLOW / XW_DOPRI_NONFINITE as xw_dopri5_attempts sets them, or XW_DOPRI_STEPS: max_steps
 *                 accepted steps without reaching t_end, or still open after max_attempts rounds (XW_DOPRI_CAPACITY does not occur)
 *   n_acc[N], n_att[N] : accepted and attempted steps
 *   Y           : NULL, or the state y(t_end) [H][N]
 *   rec, cap    : NULL, or rec[cap][2][N]: t0 and dt of each accepted step s < cap of every path (later steps are not stored;
 *                 slots past n_acc[p] are not written)
 *   fin         : NULL, or fin[2][N]: t0 and the next dt of every path's controller when it stopped (for error messages)
 * work: xw_paths_dopri5_work(d, H, K, m) doubles per 16-path tile -- the tiled dopri5 forward's, xw_tdopri5_work(0, ...) -- times
 * the launch's tiles, the sum over the jobs of (N + 15) / 16, in job order.
 * Refused on the host before any launch: XW_E_ARG for null pointers (jobs, theta, work, a job's xT, start, t_in, t_end, u, status,
 * n_acc, n_att), njobs < 1, N < 1, cap < 0 with a rec, Hn outside 1..H, a negative (or NaN) tolerance, max_steps < 1 or
 * max_attempts < 1; XW_E_DIMS where xw_tiled_ode_ok(d, H, K, m) is 0. */
#ifndef XNWAN_EVAL_H
#define XNWAN_EVAL_H
#include "xnwan.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct { const double* xT; const double* start; const double* t_in; const double* t_end; double* u; int* status; int* n_acc;
                 int* n_att; double* Y; double* rec; double* fin; int N; int cap; } XwPathsDopriJob;
int xw_paths_dopri5_work(int d, int H, int K, int m);
int xw_paths_dopri5_fwd(const XwPathsDopriJob* jobs, int njobs, const double* theta, int d, int H, int K, int m, int Hn,
                        double rtol, double atol, int max_steps, int max_attempts, double* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
