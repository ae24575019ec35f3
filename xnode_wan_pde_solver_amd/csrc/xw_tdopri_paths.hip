// xw_tdopri_paths.hip -- solver 'dopri5' at scattered space-time points: a step controller PER PATH (include/xnwan_eval.h).
//
// xw_tdopri.hip keeps one step size per JOB (one odeint call of the reference for a group of paths): every attempt is a launch, the
// tiles of a job meet in a ticket reduction and the host reads the controllers back between chunks.  Here every path is an odeint
// call of its own -- tests/dopri5_ref.py::dopri5 on the one-path group with the sample times [t_in, t_end] -- so the RMS norms run
// over the path's own u_hidden_dim entries, no tile needs another one's sums, and the whole integration of a tile is ONE launch:
// the lift, f0, both halves of _select_initial_step, the attempts with accept / reject and the next step size, FSAL, the quartic
// dense output at t_end from the accepted step that covers it, the read-out.
//
// One 64-lane wave = one workgroup = one tile of 16 paths; a path is a matrix column.  The blocks of xw_tiled_blocks.h and
// stage_input take a lane's own t and dt (kt_ode_fwd_pp of xw_tiled_paths.hip relies on the same property): their epilogues and
// element loops touch columns e & 15 == lane & 15 only.  The controller -- t0, dt, the accepted and attempted counts, the done flag
// and the status -- lives in registers per lane, the same values in the four lanes lane & 15 == p of path p: a path's norm is the
// sum of a lane's own elements in loop order, then xw_sum_over_g, which leaves one pairing's bits in all four.  The formulas are
// ctl_h0 / ctl_first_dt / ctl_next_dt of xw_dopri_ctl.h, the decisions those of ctl_init2 / ctl_attempt with N = 1.
//
// A path that is done walks along with dt = 0 (every stage is the field at (t0, y), nothing is committed); lanes past the end of
// the job copy the last path and store nothing.  A tile's loop ends when all its paths are done, or after max_attempts rounds: a
// path still open then gets XW_DOPRI_STEPS.  No float atomics, no tickets, no waits between tiles: a path's bits do not depend on its
// tile neighbours, and the launch can be captured.  The workspace is the tiled dopri5 forward's, td_work(0, ...).
//
// ckpt (include/xnwan_eval_grad.h: xw_paths_dopri5_ckpt_fwd; null from xw_paths_dopri5_fwd) keeps, per path, the state at the start
// of every accepted step below the job's cap -- what kq_paths_grad (xw_tdopri_paths_grad.hip) walks back.  Stores only: with or
// without it every other output is the same bits.
#include "xw_common.h"
#include "xnwan_eval_grad.h"

namespace {
#include "xw_generic_cot.h"   // (not used by this forward pass: the sweep helpers of xw_tiled_blocks.h name cot_u / cot_job_ok)
#include "xw_tiled_blocks.h"

__device__ __forceinline__ double gsum64(double x) { return xw_sum_over_g(xw_sum_over_n(x)); }   // (job_sum of xw_dopri_ctl.h names it)

#include "xw_dopri_ctl.h"
#include "xw_tdopri_blocks.h"

__global__ void __launch_bounds__(64) kq_paths(const XwPathsDopriJob job, const double* __restrict__ theta, int d, int H, int K, int m,
                                               int Hn, double rtol, double atol, int max_steps, int max_attempts,
                                               double* __restrict__ work, double* __restrict__ ckpt) {
  const int N = job.N, p0 = blockIdx.x * 16;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TdWork q = td_work(0, d, H, K, m);
  double* ws = work + (long)blockIdx.x * q.total;
  double* y0 = ws + q.w.hv;                                  // the state at t0
  double* yt = y0 + 16L * H;                                 // a stage's input; after stage 6 the candidate y1
  double* pre = y0 + 16L * H * 2;                            // (the lift's first pre-activation)
  double* yf = y0 + 16L * H * 3;                             // (the lift's second); then y(t_end) of every path that has got there
  double* kk = ws + q.k;                                     // k_0 .. k_6; k_0 = F(t0, y0) (FSAL)
  double* st = ws + q.w.st;
  const int l16 = lane_id() & 15;
  const int pc = p0 + l16 < N ? p0 + l16 : N - 1;            // the lane's own path
  const bool mine = lane_id() < 16 && p0 + l16 < N;          // ... and the lane that stores its scalars
  const bool keep = ckpt != nullptr && p0 + l16 < N;         // the lane stores its column's checkpoints
  const double t_end = job.t_end[pc], cnt = (double)Hn;
  if (lane_id() < 16) st[l16] = job.start[pc];
  tile_x(n, q.w, ws, job.xT, N, p0);
  tlift(n, st, pre, yf, y0);
  if (ckpt) tstore(H, N, p0, y0, ckpt);                      // slot 0: the lifted start value, of every path
  // ---- the controller, per lane: ctl_init1 / ctl_init2 with N = 1 --------------------------------------------------------------
  double t0 = job.t_in[pc];
  tfield(n, q.w, ws, t0, y0, kk, false);
  double a0 = 0.0, a1 = 0.0;
  for (int e = lane_id(); e < 16 * H; e += 64) {
    const double sc = atol + rtol * fabs(y0[e]);
    a0 += (y0[e] / sc) * (y0[e] / sc);
    a1 += (kk[e] / sc) * (kk[e] / sc);
    yf[e] = y0[e];                                           // (t_end == t_in: the read-out of y0)
  }
  const double d0 = sqrt(xw_sum_over_g(a0) / cnt), d1 = sqrt(xw_sum_over_g(a1) / cnt);
  const double h0 = ctl_h0(d0, d1);
  tcomb(H, yt, y0, h0, kk);
  tfield(n, q.w, ws, t0 + h0, yt, kk + 16L * H, false);
  double a2 = 0.0;
  for (int e = lane_id(); e < 16 * H; e += 64) {
    const double r = (kk[16L * H + e] - kk[e]) / (atol + rtol * fabs(y0[e]));
    a2 += r * r;
  }
  double dt = ctl_first_dt(d1, sqrt(xw_sum_over_g(a2) / cnt) / h0, h0);
  int nacc = 0, natt = 0, status = 0;
  bool done = !(t_end > t0);
  if (!done && !(t0 + dt > t0)) {                            // torchdiffeq: assert t0 + dt > t0, 'underflow in dt'
    status = XW_DOPRI_UNDERFLOW;
    done = true;
  }
  // ---- attempts: one round is one attempted step of every path of the tile that is not done (kq_attempt, ctl_attempt) ------------
  for (int round = 0; round < max_attempts; ++round) {
    if (__all(done)) break;                                  // (lanes past the end of the job carry the last path's flag)
    const double dte = done ? 0.0 : dt, t1 = t0 + dte;
    for (int s = 1; s < 7; ++s) {
      stage_input(H, s, dte, y0, kk, yt);
      tfield(n, q.w, ws, s == 6 ? t1 : t0 + DP_C[s] * dte, yt, kk + 16L * H * s, false);
    }
    // yt = y1 (the last stage's input, FSAL); the error estimate dt sum_j (b_j - b^_j) k_j against atol + rtol max(|y0|, |y1|)
    double ew[7], acc = 0.0;
    for (int s = 0; s < 7; ++s) ew[s] = dte * DP_E[s];
    for (int e = lane_id(); e < 16 * H; e += 64) {
      double err = 0.0;
      for (int s = 0; s < 7; ++s) err = fma(kk[16L * H * s + e], ew[s], err);
      const double r = err / (atol + rtol * fmax(fabs(y0[e]), fabs(yt[e])));
      acc += r * r;
    }
    const double ratio = sqrt(xw_sum_over_g(acc) / cnt);
    const bool open = !done;
    bool accept = false;
    double dtn = dt;
    if (open) {
      ++natt;
      if (ratio != ratio) {                                  // NaN: torchdiffeq rejects and its next dt is NaN (the underflow assert)
        status = XW_DOPRI_NONFINITE;
        done = true;
      } else {
        accept = ratio <= 1.0;
        dtn = ctl_next_dt(dt, ratio);
      }
    }
    const bool last = accept && !(t_end > t1);               // the accepted step with t0 < t_end <= t1: its dense output is y(t_end)
    double w[7];
    dense_weights(last ? (t_end - t0) / (t1 - t0) : 0.0, w);
    for (int s = 0; s < 7; ++s) w[s] *= dte;
    for (int e = lane_id(); e < 16 * H; e += 64) {
      if (last) {
        double s_ = 0.0;
        for (int s = 0; s < 7; ++s) s_ = fma(kk[16L * H * s + e], w[s], s_);
        yf[e] = y0[e] + s_;
      }
      if (accept) {                                          // commit: the candidate, and its last stage as the next k_0
        if (keep && nacc >= 1 && nacc < job.cap) ckpt[((long)nacc * H + (e >> 4)) * N + pc] = y0[e];   // slot nacc: this step's start
        y0[e] = yt[e];
        kk[e] = kk[16L * H * 6 + e];
      }
    }
    if (accept) {
      if (mine && job.rec && nacc < job.cap) {
        job.rec[(2L * nacc) * N + pc] = t0;
        job.rec[(2L * nacc + 1) * N + pc] = dte;
      }
      ++nacc;
      t0 = t1;
    }
    if (open && status == 0) {
      dt = dtn;
      if (last) {
        done = true;
      } else if (accept && nacc >= max_steps) {
        status = XW_DOPRI_STEPS;
        done = true;
      } else if (!(t0 + dt > t0)) {
        status = XW_DOPRI_UNDERFLOW;
        done = true;
      }
    }
  }
  if (!done) status = XW_DOPRI_STEPS;                        // still open after max_attempts rounds
  sync_tile();
  tput_output(n, job.u, job.Y, 0, N, p0, yf);
  if (mine) {
    job.status[pc] = status;
    job.n_acc[pc] = nacc;
    job.n_att[pc] = natt;
    if (job.fin) {
      job.fin[pc] = t0;
      job.fin[(long)N + pc] = dt;
    }
  }
}

}  // namespace

// ---- entry points (include/xnwan_eval.h) ---------------------------------------------------------------------------------------
extern "C" int xw_paths_dopri5_work(int d, int H, int K, int m) {
  if (!xw_tiled_ode_ok(d, H, K, m)) return XW_E_DIMS;
  return (int)td_work(0, d, H, K, m).total;
}

namespace {
// the checks and launches of both entry points: job i as the kernel takes it is fwd(jobs[i]) with the checkpoints ckpt(jobs[i])
template <class J, class F, class C>
int paths_fwd(const J* jobs, int njobs, F fwd, C ckpt, const double* theta, int d, int H, int K, int m, int Hn, double rtol,
              double atol, int max_steps, int max_attempts, double* work, void* stream) {
  if (!jobs || njobs < 1 || !theta || !work || !(rtol >= 0.0) || !(atol >= 0.0) || max_steps < 1 || max_attempts < 1) return XW_E_ARG;
  if (!xw_tiled_ode_ok(d, H, K, m)) return XW_E_DIMS;
  if (Hn < 1 || Hn > H) return XW_E_ARG;
  for (int i = 0; i < njobs; ++i) {
    const XwPathsDopriJob& j = fwd(jobs[i]);
    if (!j.xT || !j.start || !j.t_in || !j.t_end || !j.u || !j.status || !j.n_acc || !j.n_att || j.N < 1 || (j.rec && j.cap < 0) ||
        (ckpt(jobs[i]) && j.cap < 1))
      return XW_E_ARG;
  }
  const long per = td_work(0, d, H, K, m).total;
  long off = 0;
  for (int i = 0; i < njobs; ++i) {
    const int tiles = (fwd(jobs[i]).N + 15) / 16;
    hipLaunchKernelGGL(kq_paths, dim3(tiles), dim3(64), 0, (hipStream_t)stream, fwd(jobs[i]), theta, d, H, K, m, Hn, rtol, atol,
                       max_steps, max_attempts, work + off, ckpt(jobs[i]));
    off += per * tiles;
  }
  return xw_launch_status();
}
}  // namespace

extern "C" int xw_paths_dopri5_fwd(const XwPathsDopriJob* jobs, int njobs, const double* theta, int d, int H, int K, int m, int Hn,
                                   double rtol, double atol, int max_steps, int max_attempts, double* work, void* stream) {
  return paths_fwd(jobs, njobs, [](const XwPathsDopriJob& j) -> const XwPathsDopriJob& { return j; },
                   [](const XwPathsDopriJob&) -> double* { return nullptr; }, theta, d, H, K, m, Hn, rtol, atol, max_steps,
                   max_attempts, work, stream);
}

// ... and include/xnwan_eval_grad.h: the same launches with the checkpoints kept
extern "C" int xw_paths_dopri5_ckpt_fwd(const XwPathsDopriCkptJob* jobs, int njobs, const double* theta, int d, int H, int K, int m,
                                        int Hn, double rtol, double atol, int max_steps, int max_attempts, double* work,
                                        void* stream) {
  return paths_fwd(jobs, njobs, [](const XwPathsDopriCkptJob& j) -> const XwPathsDopriJob& { return j.f; },
                   [](const XwPathsDopriCkptJob& j) -> double* { return j.ckpt; }, theta, d, H, K, m, Hn, rtol, atol, max_steps,
                   max_attempts, work, stream);
}
