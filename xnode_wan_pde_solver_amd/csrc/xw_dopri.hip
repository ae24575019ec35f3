// xw_dopri.hip -- solver 'dopri5': torchdiffeq's adaptive Dormand-Prince 5(4) stepper with FSAL and the quartic dense output,
// the default method of torchdiffeq.odeint (src/model.py:103-106 passes config['solver'] as `method`, with no rtol / atol /
// options).  The package is absent from the reference tree: the algorithm is restated (tests/dopri5_ref.py), parity
// unpinned.
//
// One step size per JOB (one odeint call of the reference = one group of paths): every attempt needs the RMS norm of the scaled
// error over all paths x u_hidden_dim entries of the job.  Each job carries a device-side controller (ctl[XW_DOPRI_CTL], see
// include/xnwan.h); the last block of a job to finish an attempt (ticket, as grid_sum in xw_weak.hip) sums the per-block partial
// sums IN BLOCK ORDER, decides accept / reject, and advances the controller.  No float atomics, no block waits on another: the
// step decisions are bit-reproducible and no launch can hang.
//
// The field runs per path on the vector ALU (xw_generic_field.h: one lane per path, weights through the scalar cache) at the
// widths of the network's blob, so every width the stepper serves is served here too.
//
// Launches (all jobs of a launch share t):
//   kd_init1    y0 = lift(start), f0 = f(t0, y0); record slot 0, output l = 0; d0 = ||y0/scale||, d1 = ||f0/scale||, h0
//   kd_init2    d2 = ||(f(t0 + h0, y0 + h0 f0) - f0)/scale|| / h0; the first step; the controller starts
//   kd_attempt  one attempted step of every job that is not done (the host enqueues them in chunks)
//   kd_sweep    the reverse of the ACCEPTED steps, step sizes as constants (the deviation and its measured size)
#include "xw_common.h"
#include "xnwan.h"
#include "xw_generic.h"

namespace {
#include "xw_generic_field.h"
#include "xw_generic_cot.h"

#include "xw_dopri_ctl.h"

__device__ __forceinline__ void put_output(const XwDopriJob& j, const double* flw, double flb, int l, int H, int path,
                                           const double* y) {
  double acc = flb;
  for (int h = 0; h < H; ++h) acc = fma(flw[h], y[h], acc);
  j.u[(long)l * j.N + path] = acc;
  if (j.Y)
    for (int h = 0; h < H; ++h) j.Y[((long)l * H + h) * j.N + path] = y[h];
}

template <int HM>
__global__ void __launch_bounds__(64) kd_init1(const Jobs<XwDopriJob> J, const double* __restrict__ tf, const double* __restrict__ theta,
                                               int L, int d, int H, int K, int m, int Hn, double rtol, double atol) {
  int lb;
  const XwDopriJob& j = J.j[job_of(J, lb)];
  const int N = j.N, nb = (N + 63) / 64, raw = lb * 64 + (int)threadIdx.x;
  const bool active = raw < N;
  const int path = active ? raw : N - 1;
  Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  double xproj[GK], y[HM], p0[HM], p2[HM], f[HM];
  x_projection(n, j.xT, N, path, xproj);
  lift(n, j.start[path], p0, p2, y);
  field_eval(n, xproj, tf[0], y, f, nullptr);
  double acc[2] = {0.0, 0.0};
  for (int h = 0; h < H; ++h) {
    const double sc = atol + rtol * fabs(y[h]);
    acc[0] += (y[h] / sc) * (y[h] / sc);
    acc[1] += (f[h] / sc) * (f[h] / sc);
  }
  if (active) {
    for (int h = 0; h < H; ++h) {
      j.rec_y[(long)h * N + path] = y[h];
      j.fbuf[(long)h * N + path] = f[h];
    }
    const double* flw = theta + n.o.FLw;
    for (int l = 0; l < L; ++l)                             // t_0 (and sample times that do not lie past it) give y0 itself
      if (l == 0 || !(tf[l] > tf[0])) put_output(j, flw, theta[n.o.FLb], l, H, path, y);
  } else {
    acc[0] = acc[1] = 0.0;
  }
  if (job_sum<2>(acc, j.work, j.ctl, nb, lb) && threadIdx.x == 0) ctl_init1(acc, N, Hn, j.ctl);
}

template <int HM>
__global__ void __launch_bounds__(64) kd_init2(const Jobs<XwDopriJob> J, const double* __restrict__ tf, const double* __restrict__ theta,
                                               int L, int d, int H, int K, int m, int Hn, double rtol, double atol) {
  int lb;
  const XwDopriJob& j = J.j[job_of(J, lb)];
  const int N = j.N, nb = (N + 63) / 64, raw = lb * 64 + (int)threadIdx.x;
  const bool active = raw < N;
  const int path = active ? raw : N - 1;
  Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const double t0 = tf[0], h0 = j.ctl[C_H0];
  double xproj[GK], y0[HM], f0[HM], y1[HM], f1[HM];
  x_projection(n, j.xT, N, path, xproj);
  for (int h = 0; h < H; ++h) {
    y0[h] = j.rec_y[(long)h * N + path];
    f0[h] = j.fbuf[(long)h * N + path];
    y1[h] = y0[h] + h0 * f0[h];
  }
  field_eval(n, xproj, t0 + h0, y1, f1, nullptr);
  double acc[1] = {0.0};
  for (int h = 0; h < H; ++h) {
    const double r = (f1[h] - f0[h]) / (atol + rtol * fabs(y0[h]));
    acc[0] += r * r;
  }
  if (!active) acc[0] = 0.0;
  if (job_sum<1>(acc, j.work, j.ctl, nb, lb) && threadIdx.x == 0) ctl_init2(acc[0], N, Hn, tf, L, j.ctl, j.rec_t);
}

// One attempted step of every job that is not done.  The candidate y1 goes to record slot n_acc + 1 and f1 to the f buffer of the
// other parity: a rejected attempt is overwritten by the next one.  Outputs: the dense output at every sample time in (t0, t0 + dt]
// is written by EVERY attempt, accepted or not.  Correct without a separate pass: attempts start at non-decreasing t0, so the last
// attempt to write t_i is the accepted step that covers it -- every later attempt starts at or after that step's t1 >= t_i.
template <int HM>
__global__ void __launch_bounds__(64) kd_attempt(const Jobs<XwDopriJob> J, const double* __restrict__ tf,
                                                 const double* __restrict__ theta, int L, int d, int H, int K, int m, int Hn,
                                                 double rtol, double atol, int max_steps) {
  int lb;
  const XwDopriJob& j = J.j[job_of(J, lb)];
  double* c = j.ctl;
  if (c[C_DONE] != 0.0) return;                             // (uniform over the job: no block of it takes a ticket)
  const int N = j.N, nb = (N + 63) / 64, raw = lb * 64 + (int)threadIdx.x;
  const bool active = raw < N;
  const int path = active ? raw : N - 1;
  const double t0 = c[C_T0], dt = c[C_DT];
  const int na = (int)c[C_NACC];
  const bool room = na + 1 <= j.cap;                        // (the host grows the record ahead of every chunk; this only guards)
  Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  double xproj[GK], y0[HM], yt[HM], k[7][HM];
  x_projection(n, j.xT, N, path, xproj);
  const double* f0 = j.fbuf + (long)(na & 1) * H * N;
  for (int h = 0; h < H; ++h) {
    y0[h] = j.rec_y[((long)na * H + h) * N + path];
    k[0][h] = f0[(long)h * N + path];
  }
  const double t1 = t0 + dt;
  for (int s = 1; s < 7; ++s) {
    double a[6];
    for (int q = 0; q < s; ++q) a[q] = DP_A[s][q] * dt;
    for (int h = 0; h < H; ++h) {
      double acc = 0.0;
      for (int q = 0; q < s; ++q) acc = fma(k[q][h], a[q], acc);
      yt[h] = y0[h] + acc;
    }
    field_eval(n, xproj, s == 6 ? t1 : t0 + DP_C[s] * dt, yt, k[s], nullptr);
  }
  // yt = y1 (the last stage's input, FSAL); the error estimate dt sum_j (b_j - b^_j) k_j against atol + rtol max(|y0|, |y1|)
  double e[7], acc[1] = {0.0};
  for (int q = 0; q < 7; ++q) e[q] = dt * DP_E[q];
  for (int h = 0; h < H; ++h) {
    double err = 0.0;
    for (int q = 0; q < 7; ++q) err = fma(k[q][h], e[q], err);
    const double r = err / (atol + rtol * fmax(fabs(y0[h]), fabs(yt[h])));
    acc[0] += r * r;
  }
  if (active) {
    if (room) {
      double* f1 = j.fbuf + (long)((na + 1) & 1) * H * N;
      for (int h = 0; h < H; ++h) {
        j.rec_y[((long)(na + 1) * H + h) * N + path] = yt[h];
        f1[(long)h * N + path] = k[6][h];
      }
    }
    const double* flw = theta + n.o.FLw;
    for (int l = 1; l < L; ++l) {
      const double tl = tf[l];
      if (!(tl > t0 && tl <= t1)) continue;
      double w[7], p[HM];
      dense_weights((tl - t0) / (t1 - t0), w);
      for (int q = 0; q < 7; ++q) w[q] *= dt;
      for (int h = 0; h < H; ++h) {
        double s_ = 0.0;
        for (int q = 0; q < 7; ++q) s_ = fma(k[q][h], w[q], s_);
        p[h] = y0[h] + s_;
      }
      put_output(j, flw, theta[n.o.FLb], l, H, path, p);
    }
  } else {
    acc[0] = 0.0;
  }
  if (job_sum<1>(acc, j.work, c, nb, lb) && threadIdx.x == 0)
    ctl_attempt(acc[0], N, Hn, t0, dt, na, room, max_steps, tf, L, c, j.rec_t, j.rec_h);
}

// Reverse of the accepted steps (step sizes and grid constants), per path.  Step s: y_{s+1} = y_s + dt sum_j b_j k_j, stage j at
// (t_s + c_j dt, y_s + dt sum_{q<j} a_jq k_q); the outputs the step covers are p(x_i) = y_s + dt sum_j w_j(x_i) k_j.  The stages
// are recomputed from the recorded y_s (the same bits as the forward pass), their VJPs taken in reverse order.  FSAL: k_0 of step
// s is the field at (t_s, y_s), the point of k_6 of step s - 1 -- its cotangent is carried there and the VJP taken once.
template <int HM>
__global__ void __launch_bounds__(64) kd_sweep(const Jobs<XwDopriSweepJob> J, const double* __restrict__ tf,
                                               const double* __restrict__ theta, int L, int d, int H, int K, int m, int mode) {
  int lb;
  const XwDopriSweepJob& sj = J.j[job_of(J, lb)];
  const XwOdeBwdJob& job = sj.b;
  const int N = job.N;
  const int raw = lb * 64 + (int)threadIdx.x;
  const bool active = raw < N;
  const int path = active ? raw : N - 1;                       // (lanes past the end walk along with the last path, adding zeros)
  const bool want_x = (mode & 1) != 0, ones_x = (mode & 4) != 0;
  double* slab = (mode & 2) ? job.gslab + (long)(raw >> 4) * u_offsets(d, H, K).total : nullptr;
  if (slab != nullptr && (raw >> 4) * 16 >= N) slab = nullptr;  // (a group entirely past the end owns no slab)
  Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  double xproj[GK], Sx[GK], lam[HM], carry[HM], y[HM], gy[HM], a[HM], k[7][HM], kb[7][HM];
  x_projection(n, job.xT, N, path, xproj);
  for (int q = 0; q < K; ++q) Sx[q] = 0.0;
  for (int h = 0; h < H; ++h) lam[h] = carry[h] = 0.0;
  const double* flw = theta + n.o.FLw;
  const int na = (int)sj.ctl[C_NACC];
  int l = L - 1;                                               // the next output to reverse (descending)
  for (int s = na - 1; s >= 0; --s) {
    const double t0 = sj.rec_t[s], t1 = sj.rec_t[s + 1], dt = sj.rec_h[s];
    for (int h = 0; h < H; ++h) y[h] = sj.rec_y[((long)s * H + h) * N + path];
    field_eval(n, xproj, t0, y, k[0], nullptr);
    for (int st = 1; st < 7; ++st) {
      for (int h = 0; h < H; ++h) {
        double acc = 0.0;
        for (int q = 0; q < st; ++q) acc = fma(k[q][h], DP_A[st][q] * dt, acc);
        a[h] = y[h] + acc;
      }
      field_eval(n, xproj, st == 6 ? t1 : t0 + DP_C[st] * dt, a, k[st], nullptr);
    }
    // cotangents of the stages: from y_{s+1} (lam), from the outputs in (t0, t1], and (k_6) from step s + 1's k_0
    for (int q = 0; q < 7; ++q)
      for (int h = 0; h < H; ++h) kb[q][h] = dt * DP_B[q] * lam[h];
    for (int h = 0; h < H; ++h) kb[6][h] += carry[h];
    for (; l >= 1 && tf[l] > t0; --l) {
      const double ub = cot_u(job, l, L, path);
      double w[7];
      dense_weights((tf[l] - t0) / (t1 - t0), w);
      if (slab) {
        for (int h = 0; h < H; ++h) {
          double s_ = 0.0;
          for (int q = 0; q < 7; ++q) s_ = fma(k[q][h], w[q] * dt, s_);
          a[h] = y[h] + s_;                                    // the output state p(x_l)
        }
        path_readout_grad(slab, n, active, ub, a);
      }
      for (int h = 0; h < H; ++h) {
        const double yb = flw[h] * ub;
        lam[h] += yb;
        for (int q = 0; q < 7; ++q) kb[q][h] = fma(dt * w[q], yb, kb[q][h]);
      }
    }
    // stages in reverse: the VJP of stage st feeds y_s (lam) and the stages it was formed from
    for (int st = 6; st >= 0; --st) {
      if (st == 0 && s > 0) {                                  // FSAL: taken with step s - 1's k_6
        for (int h = 0; h < H; ++h) carry[h] = kb[0][h];
        break;
      }
      for (int h = 0; h < H; ++h) {
        double acc = 0.0;
        for (int q = 0; q < st; ++q) acc = fma(k[q][h], DP_A[st][q] * dt, acc);
        a[h] = y[h] + acc;
      }
      field_vjp(n, xproj, st == 6 ? t1 : t0 + DP_C[st] * dt, a, kb[st], gy, Sx, slab, active);
      for (int h = 0; h < H; ++h) {
        lam[h] += gy[h];
        for (int q = 0; q < st; ++q) kb[q][h] = fma(DP_A[st][q] * dt, gy[h], kb[q][h]);
      }
    }
  }
  // sample times that do not lie past t_0 read y0 itself
  for (; l >= 1; --l) {
    const double ub = cot_u(job, l, L, path);
    if (slab) {
      for (int h = 0; h < H; ++h) a[h] = sj.rec_y[(long)h * N + path];
      path_readout_grad(slab, n, active, ub, a);
    }
    for (int h = 0; h < H; ++h) lam[h] = fma(flw[h], ub, lam[h]);
  }
  // l = 0: read-out, then the lift 1 -> H -> H -> H (src/model.py:78) -- the tail of kg_ode_bwd (xw_generic.hip); with mode bit 2
  // the x-side outputs are those of the ALL-ONES cotangent while the parameter gradients use the job's own.  A COPY of that tail,
  // kept in step by hand: as one function for both kernels it cost kg_ode_bwd scratch and this kernel time (profiles/r19)
  const double ub0 = cot_u(job, 0, L, path);
  double p0[HM], p2[HM];
  lift(n, job.start[path], p0, p2, y);
  if (slab) path_readout_grad(slab, n, active, ub0, y);
  const double s0 = job.start[path];
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 0 && !slab) continue;
    if (pass == 1 && !(want_x && job.gs != nullptr)) continue;
    const double ub = pass == 1 && ones_x ? 1.0 : ub0;
    double l0[HM], dh2[HM], dh1[HM];
    for (int h = 0; h < H; ++h) l0[h] = fma(flw[h], ub, lam[h]);
    matvecT(theta + n.o.IL4w, H, H, H, l0, dh2);
    for (int h = 0; h < H; ++h) dh2[h] = p2[h] > 0.0 ? dh2[h] : 0.0;
    matvecT(theta + n.o.IL2w, H, H, H, dh2, dh1);
    for (int h = 0; h < H; ++h) dh1[h] = p0[h] > 0.0 ? dh1[h] : 0.0;
    if (pass == 0) {
      for (int i = 0; i < H; ++i) {
        const double li = l0[i], di = dh2[i];
        gadd_run(slab, n.o.IL4w + i * H, H, active, [&](int q) { return li * (p2[q] > 0.0 ? p2[q] : 0.0); });
        gadd_run(slab, n.o.IL2w + i * H, H, active, [&](int q) { return di * (p0[q] > 0.0 ? p0[q] : 0.0); });
      }
      gadd_run(slab, n.o.IL4b, H, active, [&](int i) { return l0[i]; });
      gadd_run(slab, n.o.IL2b, H, active, [&](int i) { return dh2[i]; });
      gadd_run(slab, n.o.IL0w, H, active, [&](int i) { return dh1[i] * s0; });
      gadd_run(slab, n.o.IL0b, H, active, [&](int i) { return dh1[i]; });
    } else if (active) {
      double acc = 0.0;
      for (int i = 0; i < H; ++i) acc = fma(theta[n.o.IL0w + i], dh1[i], acc);
      job.gs[path] = acc;
    }
  }
  const double* Win = theta + n.o.Win;
  if (slab) {
    gadd_run(slab, n.o.Winb, K, active, [&](int q) { return Sx[q]; });
    for (int q = 0; q < K; ++q) {
      const double sq = Sx[q];
      gadd_run(slab, n.o.Win + q * n.o.ldin, d, active, [&](int i) { return sq * job.xT[(long)i * N + path]; });
    }
  }
  if (want_x && job.gx != nullptr && active)
    for (int i = 0; i < d; ++i) {
      double acc = 0.0;
      for (int q = 0; q < K; ++q) acc = fma(Win[q * n.o.ldin + i], Sx[q], acc);
      job.gx[(long)i * N + path] = acc;
    }
}

bool dims_ok(int L, int d, int H, int K, int m, int Hn) { return L >= 1 && xwg_ode_ok(d, H, K, m) && Hn >= 1 && Hn <= H; }
}  // namespace

extern "C" int xw_dopri5_ctl_size(void) { return XW_DOPRI_CTL; }
extern "C" int xw_dopri5_work_size(int N) { return N < 1 ? XW_E_ARG : 2 * ((N + 63) / 64); }

extern "C" int xw_dopri5_init(const XwDopriJob* jobs, int njobs, const double* t, const double* theta, int L, int d, int H, int K,
                              int m, int Hn, double rtol, double atol, void* stream) {
  if (!t || !theta || !(rtol >= 0.0) || !(atol >= 0.0)) return XW_E_ARG;
  if (!dims_ok(L, d, H, K, m, Hn)) return XW_E_DIMS;
  Jobs<XwDopriJob> P;
  const int e = fwd_jobs(jobs, njobs, P, 64);
  if (e) return e;
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(P.blk0[njobs]), b(64);
  if (H <= 32) {
    hipLaunchKernelGGL(kd_init1<32>, g, b, 0, s, P, t, theta, L, d, H, K, m, Hn, rtol, atol);
    hipLaunchKernelGGL(kd_init2<32>, g, b, 0, s, P, t, theta, L, d, H, K, m, Hn, rtol, atol);
  } else {
    hipLaunchKernelGGL(kd_init1<64>, g, b, 0, s, P, t, theta, L, d, H, K, m, Hn, rtol, atol);
    hipLaunchKernelGGL(kd_init2<64>, g, b, 0, s, P, t, theta, L, d, H, K, m, Hn, rtol, atol);
  }
  return xw_launch_status();
}

extern "C" int xw_dopri5_attempts(const XwDopriJob* jobs, int njobs, const double* t, const double* theta, int L, int d, int H,
                                  int K, int m, int Hn, double rtol, double atol, int max_steps, int n, void* stream) {
  if (!t || !theta || !(rtol >= 0.0) || !(atol >= 0.0) || max_steps < 1 || n < 0) return XW_E_ARG;
  if (!dims_ok(L, d, H, K, m, Hn)) return XW_E_DIMS;
  Jobs<XwDopriJob> P;
  const int e = fwd_jobs(jobs, njobs, P, 64);
  if (e) return e;
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(P.blk0[njobs]), b(64);
  for (int i = 0; i < n; ++i) {
    if (H <= 32)
      hipLaunchKernelGGL(kd_attempt<32>, g, b, 0, s, P, t, theta, L, d, H, K, m, Hn, rtol, atol, max_steps);
    else
      hipLaunchKernelGGL(kd_attempt<64>, g, b, 0, s, P, t, theta, L, d, H, K, m, Hn, rtol, atol, max_steps);
  }
  return xw_launch_status();
}

extern "C" int xw_dopri5_sweep(const XwDopriSweepJob* jobs, int njobs, const double* t, const double* theta, int L, int d, int H,
                               int K, int m, int mode, void* stream) {
  if (!t || !theta || L < 1 || (mode & ~7) || ((mode & 4) && (mode & 3) != 3)) return XW_E_ARG;
  if (!xwg_ode_ok(d, H, K, m)) return XW_E_DIMS;
  Jobs<XwDopriSweepJob> P;
  hipStream_t s = (hipStream_t)stream;
  const int e = sweep_jobs(jobs, njobs, P, mode, u_offsets(d, H, K).total, 64, true, s);
  if (e) return e;
  const dim3 g(P.blk0[njobs]), b(64);
  if (H <= 32)
    hipLaunchKernelGGL(kd_sweep<32>, g, b, 0, s, P, t, theta, L, d, H, K, m, mode);
  else
    hipLaunchKernelGGL(kd_sweep<64>, g, b, 0, s, P, t, theta, L, d, H, K, m, mode);
  return xw_launch_status();
}
