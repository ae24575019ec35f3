// xw_tdopri_paths_grad.hip -- solver 'dopri5' at scattered space-time points: the reverse sweep over every path's OWN record, the
// cotangent 1 on every path's value u_p = FL(y_p(t_end)) (include/xnwan_eval_grad.h).
//
// kq_paths (xw_tdopri_paths.hip, through xw_paths_dopri5_ckpt_fwd) has written, per path, the count n_acc, t0 and dt of every
// accepted step (rec) and the state at its start (ckpt); this kernel never runs a controller.  It is kq_sweep of xw_tdopri.hip --
// the reverse of a Dormand-Prince step from the recorded y_s, the stages recomputed and their VJPs taken in reverse order, the
// dense-output cotangents, the FSAL carry -- with what kq_sweep reads per JOB held per LANE, as kt_paths_grad (xw_tiled_paths_grad.hip)
// holds a fixed grid: one wave per 16-path tile, the workspace of the tiled dopri5 sweep (td_work(1, ...)), the lane's own path in
// column lane & 15, its count, t0 and dt in registers.  The blocks of xw_tiled_blocks.h and stage_input take them by value.
//
// The tile walks s = S - 1 .. 0, S the largest count among its real paths.  For a path with na accepted steps:
//   s == na - 1  the step that covers t_end: u = FL(y_s + dt sum_j w_j(x) k_j), x = (t_end - t0) / (t1 - t0) -- the forward's
//                expression.  lam = FL_w is the cotangent of y_s, the stage cotangents are dt w_j(x) lam, nothing comes through y_{s+1}
//   s <  na - 1  y_{s+1} = y_s + dt sum_j b_j k_j: stage cotangents dt b_j lam, and k_6 takes the carried cotangent of step s + 1's
//                k_0 (FSAL: the same field value; its VJP is taken once, only step 0 takes its own)
//   s >= na      the path has no such step: dt = 0 and the state of its last own slot (slot 0 without steps).  Every stage
//                cotangent is 0 * lam, every VJP adds exact zeros to lam, Sx and the carry: the round is the identity, and a
//                path's bits do not depend on the paths beside it.  t0 and dt of such a lane come from a select, never from
//                memory -- slots at or past n_acc are not written by the forward and may hold anything, NaN included
// The checkpoint load is per COLUMN: element e of the tile belongs to column e & 15 == lane & 15, whose path has its own slot.
//
// The tail is kt_paths_grad's: the lift reversed for gs, Win^T Sx for gx; ut = FL_w . F(t_end, x, Y) is the CONTINUOUS model's time
// derivative.  No parameter gradients (slab == nullptr throughout).  Lanes past the end of a job walk with the last path and store
// nothing.  No float atomics, no waits between tiles, no read-back: the launch can be captured.
#include "xw_common.h"
#include "xnwan_eval_grad.h"

namespace {
#include "xw_generic_cot.h"   // (not used by this sweep: the sweep helpers of xw_tiled_blocks.h name cot_u / cot_job_ok)
#include "xw_tiled_blocks.h"

__device__ __forceinline__ double gsum64(double x) { return xw_sum_over_g(xw_sum_over_n(x)); }   // (job_sum of xw_dopri_ctl.h names it)

#include "xw_dopri_ctl.h"
#include "xw_tdopri_blocks.h"

__device__ __forceinline__ int clamp_count(int na, int cap) { return na < 0 ? 0 : (na > cap ? cap : na); }

__global__ void __launch_bounds__(64) kq_paths_grad(const XwPathsDopriGradJob job, const double* __restrict__ theta, int d, int H, int K,
                                                    int m, double* __restrict__ work) {
  const int N = job.N, p0 = blockIdx.x * 16;
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
  double* dh2 = hv + 16L * H * 8;
  double* dh1 = hv + 16L * H * 9;
  double* kk = ws + q.k;
  double* kb = kk + 16L * H * 7;
  double* st = ws + w.st;
  double* Sx = ws + w.total - 16L * K;
  const int l16 = lane_id() & 15;
  const int pc = p0 + l16 < N ? p0 + l16 : N - 1;                 // the lane's own path
  const double* flw = theta + n.o.FLw;
  const int na = clamp_count(job.n_acc[pc], job.cap);             // ... and its count
  const double t_in = job.t_in[pc], t_end = job.t_end[pc];
  int S = 0;                                                      // the tile's rounds
  for (int c = 0; c < 16 && p0 + c < N; ++c) {
    const int nc = clamp_count(job.n_acc[p0 + c], job.cap);
    S = nc > S ? nc : S;
  }
  // prologue: the start values, Sx = 0, no carry, lam = FL_w (the cotangent 1 on u), the tile's x and xproj
  if (lane_id() < 16) st[l16] = job.start[pc];
  for (int e = lane_id(); e < 16 * K; e += 64) Sx[e] = 0.0;
  for (int e = lane_id(); e < 16 * H; e += 64) {
    lam[e] = flw[e >> 4];
    carry[e] = 0.0;
  }
  tile_x(n, w, ws, job.xT, N, p0);
  if (job.ut) {                                                    // ut = FL_w . F(t_end, x, Y)
    tload(H, N, p0, job.Y, y);
    sync_tile();
    tfield(n, w, ws, t_end, y, gy, false);
    if (lane_id() < 16 && p0 + l16 < N) {
      double s_ = 0.0;
      for (int h = 0; h < H; ++h) s_ = fma(flw[h], gy[h * 16 + l16], s_);
      job.ut[p0 + l16] = s_;
    }
    sync_tile();
  }
  if (!(job.gx || job.gs)) return;
  for (int s = S - 1; s >= 0; --s) {
    const bool own = s < na, last = s == na - 1;
    const int slot = own ? s : (na > 0 ? na - 1 : 0);             // a slot the path owns
    double t0 = t_in, dt = 0.0;
    if (own) {
      t0 = job.rec[(2L * s) * N + pc];
      dt = job.rec[(2L * s + 1) * N + pc];
    }
    const double t1 = t0 + dt;
    for (int e = lane_id(); e < 16 * H; e += 64) y[e] = job.ckpt[((long)slot * H + (e >> 4)) * N + pc];
    sync_tile();
    tfield(n, w, ws, t0, y, kk, true);
    for (int sg = 1; sg < 7; ++sg) {
      stage_input(H, sg, dt, y, kk, a);
      tfield(n, w, ws, sg == 6 ? t1 : t0 + DP_C[sg] * dt, a, kk + 16L * H * sg, true);
    }
    // cotangents of the stages: from the dense output at t_end (the path's last step) or from y_{s+1}, and (k_6) from step s + 1's k_0
    double c[7];
    dense_weights(last ? (t_end - t0) / (t1 - t0) : 0.0, c);
    for (int g = 0; g < 7; ++g) c[g] = dt * (last ? c[g] : DP_B[g]);
    for (int e = lane_id(); e < 16 * H; e += 64) {
      for (int g = 0; g < 7; ++g) kb[16L * H * g + e] = c[g] * lam[e];
      kb[16L * H * 6 + e] += carry[e];
    }
    // stages in reverse: the VJP of stage sg feeds y_s (lam) and the stages it was formed from
    for (int sg = 6; sg >= 0; --sg) {
      if (sg == 0 && s > 0) {                                      // FSAL: taken with step s - 1's k_6
        for (int e = lane_id(); e < 16 * H; e += 64) carry[e] = kb[e];
        break;
      }
      stage_input(H, sg, dt, y, kk, a);
      tfield_vjp(n, w, ws, sg == 6 ? t1 : t0 + DP_C[sg] * dt, a, kb + 16L * H * sg, gy, nullptr);
      for (int e = lane_id(); e < 16 * H; e += 64) {
        const double g_ = gy[e];
        lam[e] += g_;
        for (int g = 0; g < sg; ++g) kb[16L * H * g + e] = fma(DP_A[sg][g] * dt, g_, kb[16L * H * g + e]);
      }
    }
    sync_tile();
  }
  // tail (kt_paths_grad's): the lift 1 -> H -> H -> H reversed for gs, Win^T Sx for gx.  lam is the whole cotangent of y_0: the
  // steps' share and the read-out's own (FL_w, set above; alone for a path without steps)
  if (job.gs) {
    tlift(n, st, p0v, p2v, y0);
    tgemm(theta + n.o.IL4w, 1, H, H, H, lam, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p2v, dh2);
    tgemm(theta + n.o.IL2w, 1, H, H, H, dh2, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p0v, dh1);
    if (lane_id() < 16 && p0 + l16 < N) {
      double s_ = 0.0;
      for (int i = 0; i < H; ++i) s_ = fma(theta[n.o.IL0w + i], dh1[i * 16 + l16], s_);
      job.gs[p0 + l16] = s_;
    }
  }
  if (job.gx) {
    double* gxt = ws + w.xt + 16L * d;
    tgemm(theta + n.o.Win, 1, n.o.ldin, d, K, Sx, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, gxt);
    tstore(d, N, p0, gxt, job.gx);
  }
}

}  // namespace

// ---- entry points (include/xnwan_eval_grad.h; xw_paths_dopri5_ckpt_fwd is beside its kernel in xw_tdopri_paths.hip) ----------------
extern "C" int xw_paths_dopri5_grad_work(int d, int H, int K, int m) { return xw_tdopri5_work(1, d, H, K, m); }

extern "C" int xw_paths_dopri5_grad(const XwPathsDopriGradJob* jobs, int njobs, const double* theta, int d, int H, int K, int m,
                                    double* work, void* stream) {
  if (!jobs || njobs < 1 || !theta || !work) return XW_E_ARG;
  if (!xw_tiled_ode_ok(d, H, K, m)) return XW_E_DIMS;
  for (int i = 0; i < njobs; ++i) {
    const XwPathsDopriGradJob& j = jobs[i];
    if (!j.xT || !j.start || !j.t_in || !j.t_end || !j.n_acc || !j.rec || !j.ckpt || !(j.gx || j.gs || j.ut) || (j.ut && !j.Y) ||
        j.N < 1 || j.cap < 1)
      return XW_E_ARG;
  }
  const long per = td_work(1, d, H, K, m).total;
  long off = 0;
  for (int i = 0; i < njobs; ++i) {
    const int tiles = (jobs[i].N + 15) / 16;
    hipLaunchKernelGGL(kq_paths_grad, dim3(tiles), dim3(64), 0, (hipStream_t)stream, jobs[i], theta, d, H, K, m, work + off);
    off += per * tiles;
  }
  return xw_launch_status();
}
