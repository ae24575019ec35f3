// xw_tdopri.hip -- solver 'dopri5' on the TILED stepper family: the second implementation of the adaptive Dormand-Prince 5(4)
// stepper of xw_dopri.hip (same algorithm, controller, record, status codes and deviations: DESIGN 8), with the field on the matrix
// pipe at the network's own runtime widths, u_hidden_dim H <= 256, u_hidden_hidden_dim K <= 256, u_layers 1..32.
//
// One 64-lane wave = one workgroup = one tile of 16 paths; every layer of the field is a product on v_mfma_f64_16x16x4 written with
// the building blocks of xw_tiled_blocks.h (tgemm / touter / trowsum / tfield / tfield_vjp / tile_x / tlift / tcomb / tload / tstore).  The tile's
// vectors are [rows][16] doubles in a per-tile slice of a caller-provided workspace (xw_tdopri5_work: the family's TileWork, and
// behind it the stages k_0 .. k_6 -- in the sweep also their cotangents); phases are ordered by sync_tile().  The workspace is per
// LAUNCH: nothing in it is read by a later launch.  In particular xproj = Win[:, 0..d) x + Win.b is recomputed by every launch
// (one [K x d] product against six or thirteen whole field evaluations) and not kept with the record, so a record stays what it
// is in xw_dopri.hip and either implementation's sweep can reverse either implementation's forward pass.
//
// One step size per JOB: every attempt needs the RMS norm of the scaled error over all paths x u_hidden_dim entries of the job.
// The tile's partial sums go through job_sum (xw_dopri_ctl.h) unchanged -- plain stores, release fence, ticket, the last tile to
// arrive sums the partials IN TILE ORDER and advances the controller -- with one partial per TILE (xw_tdopri5_part_size).  No float
// atomics, no tile waits on another: the step decisions are the same bits on every run and no launch can hang.  The summation order
// differs from xw_dopri.hip's (per 16 paths, rows in steps of four), so the two implementations agree to rounding, not to the bit.
//
// Lanes of a tile past the end of a job walk along with the last path: they add exact zeros to every norm and to every gradient,
// and store nothing.  At the fused containers' widths the kernels run at the blob's widths with Hn = the network's u_hidden_dim
// as the RMS divisor; zero-padded rows contribute zeros.
//
// Launches (all jobs of a launch share t):
//   kq_init1    y0 = lift(start), f0 = F(t0, y0); record slot 0, output l = 0; d0 = ||y0/scale||, d1 = ||f0/scale||, h0
//   kq_init2    d2 = ||(F(t0 + h0, y0 + h0 f0) - f0)/scale|| / h0; the first step; the controller starts
//   kq_attempt  one attempted step of every job that is not done (the host enqueues them in chunks)
//   kq_sweep    the reverse of the ACCEPTED steps, step sizes as constants; prologue and tail are the family's (sweep_prologue, sweep_tail)
#include "xw_common.h"
#include "xnwan.h"

namespace {
#include "xw_generic_cot.h"
#include "xw_tiled_blocks.h"

__device__ __forceinline__ double gsum64(double x) { return xw_sum_over_g(xw_sum_over_n(x)); }   // sum over the wave

#include "xw_dopri_ctl.h"
#include "xw_tdopri_blocks.h"   // the per-tile workspace (td_work) and the input of a stage (stage_input)

__global__ void __launch_bounds__(64) kq_init1(const Jobs<XwDopriJob> J, const double* __restrict__ tf, const double* __restrict__ theta,
                                               int L, int d, int H, int K, int m, int Hn, double rtol, double atol,
                                               double* __restrict__ work) {
  int lb;
  const XwDopriJob& j = J.j[job_of(J, lb)];
  const int N = j.N, nb = (N + 15) / 16, p0 = lb * 16;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TdWork q = td_work(0, d, H, K, m);
  double* ws = work + (long)blockIdx.x * q.total;
  double* y = ws + q.w.hv;
  double* pre0 = y + 16L * H * 2;
  double* pre2 = y + 16L * H * 3;
  double* f = ws + q.k;
  double* st = ws + q.w.st;
  const int l16 = lane_id() & 15;
  if (lane_id() < 16) st[l16] = j.start[p0 + l16 < N ? p0 + l16 : N - 1];
  tile_x(n, q.w, ws, j.xT, N, p0);
  tlift(n, st, pre0, pre2, y);
  tfield(n, q.w, ws, tf[0], y, f, false);
  double acc[2] = {0.0, 0.0};
  for (int e = lane_id(); e < 16 * H; e += 64) {
    if (p0 + (e & 15) >= N) continue;
    const double sc = atol + rtol * fabs(y[e]);
    acc[0] += (y[e] / sc) * (y[e] / sc);
    acc[1] += (f[e] / sc) * (f[e] / sc);
  }
  tstore(H, N, p0, y, j.rec_y);
  tstore(H, N, p0, f, j.fbuf);
  for (int l = 0; l < L; ++l)                               // t_0 (and sample times that do not lie past it) give y0 itself
    if (l == 0 || !(tf[l] > tf[0])) tput_output(n, j.u, j.Y, l, N, p0, y);
  if (job_sum<2>(acc, j.work, j.ctl, nb, lb) && threadIdx.x == 0) ctl_init1(acc, N, Hn, j.ctl);
}

__global__ void __launch_bounds__(64) kq_init2(const Jobs<XwDopriJob> J, const double* __restrict__ tf, const double* __restrict__ theta,
                                               int L, int d, int H, int K, int m, int Hn, double rtol, double atol,
                                               double* __restrict__ work) {
  int lb;
  const XwDopriJob& j = J.j[job_of(J, lb)];
  const int N = j.N, nb = (N + 15) / 16, p0 = lb * 16;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TdWork q = td_work(0, d, H, K, m);
  double* ws = work + (long)blockIdx.x * q.total;
  double* y0 = ws + q.w.hv;
  double* y1 = y0 + 16L * H;
  double* f0 = ws + q.k;
  double* f1 = f0 + 16L * H;
  const double t0 = tf[0], h0 = j.ctl[C_H0];
  tload(H, N, p0, j.rec_y, y0);
  tload(H, N, p0, j.fbuf, f0);
  tile_x(n, q.w, ws, j.xT, N, p0);
  tcomb(H, y1, y0, h0, f0);
  tfield(n, q.w, ws, t0 + h0, y1, f1, false);
  double acc[1] = {0.0};
  for (int e = lane_id(); e < 16 * H; e += 64) {
    if (p0 + (e & 15) >= N) continue;
    const double r = (f1[e] - f0[e]) / (atol + rtol * fabs(y0[e]));
    acc[0] += r * r;
  }
  if (job_sum<1>(acc, j.work, j.ctl, nb, lb) && threadIdx.x == 0) ctl_init2(acc[0], N, Hn, tf, L, j.ctl, j.rec_t);
}

// One attempted step of every job that is not done (kd_attempt of xw_dopri.hip on tiles).  The candidate y1 goes to record slot
// n_acc + 1 and f1 to the f buffer of the other parity: a rejected attempt is overwritten by the next one.  The dense output at
// every sample time in (t0, t0 + dt] is written by EVERY attempt, accepted or not: attempts start at non-decreasing t0, so the last
// attempt to write t_i is the accepted step that covers it.
__global__ void __launch_bounds__(64) kq_attempt(const Jobs<XwDopriJob> J, const double* __restrict__ tf,
                                                 const double* __restrict__ theta, int L, int d, int H, int K, int m, int Hn,
                                                 double rtol, double atol, int max_steps, double* __restrict__ work) {
  int lb;
  const XwDopriJob& j = J.j[job_of(J, lb)];
  double* c = j.ctl;
  if (c[C_DONE] != 0.0) return;                             // (uniform over the job: no tile of it takes a ticket)
  const int N = j.N, nb = (N + 15) / 16, p0 = lb * 16;
  const double t0 = c[C_T0], dt = c[C_DT];
  const int na = (int)c[C_NACC];
  const bool room = na + 1 <= j.cap;                        // (the host grows the record ahead of every chunk; this only guards)
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TdWork q = td_work(0, d, H, K, m);
  double* ws = work + (long)blockIdx.x * q.total;
  double* y0 = ws + q.w.hv;
  double* yt = y0 + 16L * H;
  double* pv = y0 + 16L * H * 2;
  double* kk = ws + q.k;
  tload(H, N, p0, j.rec_y + (long)na * H * N, y0);
  tload(H, N, p0, j.fbuf + (long)(na & 1) * H * N, kk);
  tile_x(n, q.w, ws, j.xT, N, p0);
  const double t1 = t0 + dt;
  for (int s = 1; s < 7; ++s) {
    stage_input(H, s, dt, y0, kk, yt);
    tfield(n, q.w, ws, s == 6 ? t1 : t0 + DP_C[s] * dt, yt, kk + 16L * H * s, false);
  }
  // yt = y1 (the last stage's input, FSAL); the error estimate dt sum_j (b_j - b^_j) k_j against atol + rtol max(|y0|, |y1|)
  double ew[7], acc[1] = {0.0};
  for (int s = 0; s < 7; ++s) ew[s] = dt * DP_E[s];
  for (int e = lane_id(); e < 16 * H; e += 64) {
    if (p0 + (e & 15) >= N) continue;
    double err = 0.0;
    for (int s = 0; s < 7; ++s) err = fma(kk[16L * H * s + e], ew[s], err);
    const double r = err / (atol + rtol * fmax(fabs(y0[e]), fabs(yt[e])));
    acc[0] += r * r;
  }
  if (room) {
    tstore(H, N, p0, yt, j.rec_y + (long)(na + 1) * H * N);
    tstore(H, N, p0, kk + 16L * H * 6, j.fbuf + (long)((na + 1) & 1) * H * N);
  }
  for (int l = 1; l < L; ++l) {
    const double tl = tf[l];
    if (!(tl > t0 && tl <= t1)) continue;
    double w[7];
    dense_weights((tl - t0) / (t1 - t0), w);
    for (int s = 0; s < 7; ++s) w[s] *= dt;
    for (int e = lane_id(); e < 16 * H; e += 64) {
      double s_ = 0.0;
      for (int s = 0; s < 7; ++s) s_ = fma(kk[16L * H * s + e], w[s], s_);
      pv[e] = y0[e] + s_;
    }
    sync_tile();
    tput_output(n, j.u, j.Y, l, N, p0, pv);
    sync_tile();
  }
  if (job_sum<1>(acc, j.work, c, nb, lb) && threadIdx.x == 0)
    ctl_attempt(acc[0], N, Hn, t0, dt, na, room, max_steps, tf, L, c, j.rec_t, j.rec_h);
}

// Reverse of the accepted steps (step sizes and grid constants), per tile: kd_sweep of xw_dopri.hip on tiles.  Step s:
// y_{s+1} = y_s + dt sum_j b_j k_j, stage j at (t_s + c_j dt, y_s + dt sum_{q<j} a_jq k_q); the outputs the step covers are
// p(x_i) = y_s + dt sum_j w_j(x_i) k_j.  The stages are recomputed from the recorded y_s, their VJPs taken in reverse order.
// FSAL: k_0 of step s is the field at (t_s, y_s), the point of k_6 of step s - 1 -- its cotangent is carried there and the VJP taken
// once; only step 0 takes its own.
__global__ void __launch_bounds__(64) kq_sweep(const Jobs<XwDopriSweepJob> J, const double* __restrict__ tf,
                                               const double* __restrict__ theta, int L, int d, int H, int K, int m, int mode,
                                               double* __restrict__ work) {
  int lb;
  const XwDopriSweepJob& sj = J.j[job_of(J, lb)];
  const XwOdeBwdJob& job = sj.b;
  const int N = job.N, p0 = lb * 16;
  double* slab = (mode & 2) ? job.gslab + (long)lb * u_offsets(d, H, K).total : nullptr;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TdWork q = td_work(1, d, H, K, m);
  const TileWork& w = q.w;
  double* ws = work + (long)blockIdx.x * q.total;
  double* hv = ws + w.hv;
  double* lam = hv;
  double* carry = hv + 16L * H * 1;
  double* y = hv + 16L * H * 2;
  double* gy = hv + 16L * H * 3;
  double* a = hv + 16L * H * 4;
  double* p0v = hv + 16L * H * 5;
  double* p2v = hv + 16L * H * 6;
  double* y0 = hv + 16L * H * 7;
  double* l0 = hv + 16L * H * 8;
  double* dh2 = hv + 16L * H * 9;
  double* dh1 = hv + 16L * H * 10;
  double* kk = ws + q.k;
  double* kb = kk + 16L * H * 7;
  double* ub = ws + w.ub;
  for (int e = lane_id(); e < 16 * H; e += 64) carry[e] = 0.0;
  sweep_prologue(n, w, ws, job, p0, lam);
  const double* flw = theta + n.o.FLw;
  const int na = (int)sj.ctl[C_NACC];
  int l = L - 1;                                               // the next output to reverse (descending)
  for (int s = na - 1; s >= 0; --s) {
    const double t0 = sj.rec_t[s], t1 = sj.rec_t[s + 1], dt = sj.rec_h[s];
    tload(H, N, p0, sj.rec_y + (long)s * H * N, y);
    sync_tile();
    tfield(n, w, ws, t0, y, kk, true);
    for (int sg = 1; sg < 7; ++sg) {
      stage_input(H, sg, dt, y, kk, a);
      tfield(n, w, ws, sg == 6 ? t1 : t0 + DP_C[sg] * dt, a, kk + 16L * H * sg, true);
    }
    // cotangents of the stages: from y_{s+1} (lam), from the outputs in (t0, t1], and (k_6) from step s + 1's k_0
    for (int e = lane_id(); e < 16 * H; e += 64) {
      for (int g = 0; g < 7; ++g) kb[16L * H * g + e] = dt * DP_B[g] * lam[e];
      kb[16L * H * 6 + e] += carry[e];
    }
    for (; l >= 1 && tf[l] > t0; --l) {
      tcot_ub(job, l, L, p0, ub);
      double dw[7];
      dense_weights((tf[l] - t0) / (t1 - t0), dw);
      if (slab)
        for (int e = lane_id(); e < 16 * H; e += 64) {
          double s_ = 0.0;
          for (int g = 0; g < 7; ++g) s_ = fma(kk[16L * H * g + e], dw[g] * dt, s_);
          a[e] = y[e] + s_;                                    // the output state p(x_l)
        }
      sync_tile();
      if (slab) readout_grad(slab, n, a, ub);
      for (int e = lane_id(); e < 16 * H; e += 64) {
        const double yb = flw[e >> 4] * ub[e & 15];
        lam[e] += yb;
        for (int g = 0; g < 7; ++g) kb[16L * H * g + e] = fma(dt * dw[g], yb, kb[16L * H * g + e]);
      }
      sync_tile();
    }
    // stages in reverse: the VJP of stage sg feeds y_s (lam) and the stages it was formed from
    for (int sg = 6; sg >= 0; --sg) {
      if (sg == 0 && s > 0) {                                  // FSAL: taken with step s - 1's k_6
        for (int e = lane_id(); e < 16 * H; e += 64) carry[e] = kb[e];
        break;
      }
      stage_input(H, sg, dt, y, kk, a);
      tfield_vjp(n, w, ws, sg == 6 ? t1 : t0 + DP_C[sg] * dt, a, kb + 16L * H * sg, gy, slab);
      for (int e = lane_id(); e < 16 * H; e += 64) {
        const double g_ = gy[e];
        lam[e] += g_;
        for (int g = 0; g < sg; ++g) kb[16L * H * g + e] = fma(DP_A[sg][g] * dt, g_, kb[16L * H * g + e]);
      }
    }
    sync_tile();
  }
  // sample times that do not lie past t_0 read y0 itself
  for (; l >= 1; --l) {
    if (slab) tload(H, N, p0, sj.rec_y, a);
    tcot_output(job, n, l, L, p0, ub, a, lam, slab);
  }
  sweep_tail(n, w, ws, job, L, p0, mode, slab, lam, p0v, p2v, y0, l0, dh2, dh1);
}

bool dims_ok(int d, int H, int K, int m) { return xw_tiled_ode_ok(d, H, K, m) != 0; }   // the family's widths and depths

// the scalar arguments of the forward launches, before any job is read
int fwd_check(int njobs, const double* t, const double* theta, int L, int d, int H, int K, int m, int Hn, double rtol, double atol,
              const double* work) {
  if (!t || !theta || !work || L < 1 || njobs < 1 || njobs > XW_DOPRI_MAXJOBS || !(rtol >= 0.0) || !(atol >= 0.0)) return XW_E_ARG;
  if (!dims_ok(d, H, K, m)) return XW_E_DIMS;
  if (Hn < 1 || Hn > H) return XW_E_ARG;
  return 0;
}
}  // namespace

extern "C" int xw_tdopri5_work(int sweep, int d, int H, int K, int m) {
  if (!dims_ok(d, H, K, m)) return XW_E_DIMS;
  return (int)td_work(sweep != 0, d, H, K, m).total;
}

extern "C" int xw_tdopri5_part_size(int N) { return N < 1 ? XW_E_ARG : 2 * ((N + 15) / 16); }

extern "C" int xw_tdopri5_init(const XwDopriJob* jobs, int njobs, const double* t, const double* theta, int L, int d, int H, int K,
                               int m, int Hn, double rtol, double atol, double* work, void* stream) {
  int e = fwd_check(njobs, t, theta, L, d, H, K, m, Hn, rtol, atol, work);
  if (e) return e;
  Jobs<XwDopriJob> P;
  e = fwd_jobs(jobs, njobs, P, 16);
  if (e) return e;
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(P.blk0[njobs]), b(64);
  hipLaunchKernelGGL(kq_init1, g, b, 0, s, P, t, theta, L, d, H, K, m, Hn, rtol, atol, work);
  hipLaunchKernelGGL(kq_init2, g, b, 0, s, P, t, theta, L, d, H, K, m, Hn, rtol, atol, work);
  return xw_launch_status();
}

extern "C" int xw_tdopri5_attempts(const XwDopriJob* jobs, int njobs, const double* t, const double* theta, int L, int d, int H,
                                   int K, int m, int Hn, double rtol, double atol, int max_steps, int n, double* work,
                                   void* stream) {
  int e = fwd_check(njobs, t, theta, L, d, H, K, m, Hn, rtol, atol, work);
  if (e) return e;
  if (max_steps < 1 || n < 0) return XW_E_ARG;
  Jobs<XwDopriJob> P;
  e = fwd_jobs(jobs, njobs, P, 16);
  if (e) return e;
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(P.blk0[njobs]), b(64);
  for (int i = 0; i < n; ++i)
    hipLaunchKernelGGL(kq_attempt, g, b, 0, s, P, t, theta, L, d, H, K, m, Hn, rtol, atol, max_steps, work);
  return xw_launch_status();
}

extern "C" int xw_tdopri5_sweep(const XwDopriSweepJob* jobs, int njobs, const double* t, const double* theta, int L, int d, int H,
                                int K, int m, int mode, double* work, void* stream) {
  if (!t || !theta || !work || L < 1 || njobs < 1 || njobs > XW_DOPRI_MAXJOBS) return XW_E_ARG;
  if ((mode & 3) == 0 || (mode & ~31) || ((mode & 4) && (mode & 3) != 3)) return XW_E_ARG;
  if (!dims_ok(d, H, K, m) || (mode & (8 | 16))) return XW_E_DIMS;   // (no continuous adjoint, no narrow tiles in this family)
  Jobs<XwDopriSweepJob> P;
  hipStream_t s = (hipStream_t)stream;
  const int e = sweep_jobs(jobs, njobs, P, mode, u_offsets(d, H, K).total, 16, false, s);
  if (e) return e;
  hipLaunchKernelGGL(kq_sweep, dim3(P.blk0[njobs]), dim3(64), 0, s, P, t, theta, L, d, H, K, m, mode, work);
  return xw_launch_status();
}
