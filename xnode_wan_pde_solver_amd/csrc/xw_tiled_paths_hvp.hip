// xw_tiled_paths_hvp.hip -- second derivatives of u over a RAGGED group: the Hessian of every path's final value U_p(x, s) =
// FL(y_{n_p}) in (x, start), applied to a direction (vx_p, vs_p) of the path's own (include/xnwan_hess.h).  Forward over reverse:
// the tangent of kt_paths_grad's chain (xw_tiled_paths_grad.hip) along the direction.
//
// The lift and the hidden layers of the field are ReLU -- piecewise linear, their gates constants of the differentiation, as
// autograd takes them -- so the one curvature of the model is the tanh in front of the field's output layer: the tangent of the VJP
// chain is the same chain on a second top vector plus one elementwise term (tfield_vjp_tan).  Two kernels, one wave per 16-path
// tile each, t0 and dt in a register per lane as in kt_paths_grad, every product on tgemm (xw_tiled_blocks.h):
//   kt_paths_jvp  walks the checkpoints Y[L][H][N] of kt_ode_fwd_pp (not last_only) FORWARD: the stages inside a step are recomputed
//                 from Y[l - 1], the primal trajectory never; it writes the tangent checkpoints Yd[L][H][N] (every row: the rows
//                 behind the tile's last step hold the final tangent, as Y's hold the final state) and ju = FL_w . yd_final.
//   kt_paths_hvp  walks Y and Yd BACK, carrying lam, Sx (kt_paths_grad's, recomputed: the second-order term needs them) and their
//                 tangents lamd, Sxd; the tail gives hx = Win[:, :d]^T Sxd and hs, the lift's reverse chain on lamd (the lift is
//                 piecewise linear: no second-order term of its own).
// A zero-length step is the exact identity for yd, lamd and Sxd as it is for y, lam and Sx (0 * finite, exact zeros added), so a
// path's bits depend neither on its tile neighbours nor on the nstep hint, and a path without a step has hx = hs = 0 exactly.
// Time is not perturbed.  Lanes past the end of a job walk with the last path and store nothing.  No LDS, no float atomics, no
// waits between blocks, no read-back: both launches can be captured.
// The workspace is this family's own (hvp_work, xw_tiled_paths_blocks.h, with tfield_tan, tfield_vjp_tan, tile_steps and
// hvp_prologue: shared with xw_tiled_paths_gvjp.hip): the tiled sweep's (tile_work(1, ...), which the blocks of xw_tiled_blocks.h
// address) with the tangent vectors behind it.
#include "xw_common.h"
#include "xnwan_hess.h"

namespace {
#include "xw_generic_cot.h"   // (not used here: the sweep helpers of xw_tiled_blocks.h name cot_u / cot_job_ok)
#include "xw_tiled_blocks.h"
#include "xw_tiled_paths_blocks.h"   // HvpWork, tfield_tan, tfield_vjp_tan, tile_steps, hvp_prologue (shared with xw_tiled_paths_gvjp.hip)

// tstep_rk4_bwd with its tangent: v.lam and vd.lam, the cotangent of y_l and its tangent, become those of y_{l-1} (v.Y1, vd.Y1)
__device__ void tstep_rk4_bwd_tan(const Net& n, const TileWork& w, const HvpWork& x, double* ws, double t0, double dt, const SweepVecs& v,
                                  const SweepVecs& vd) {
  const int H = n.H;
  tfield(n, w, ws, t0, v.Y1, v.fo, true);                            // k1; cc = k1
  tfield_tan(n, w, x, ws, vd.Y1, vd.fo);
  tcomb(H, v.cc, nullptr, 1.0, v.fo);
  tcomb(H, vd.cc, nullptr, 1.0, vd.fo);
  tcomb(H, v.Y2, v.Y1, dt / 3, v.fo);
  tcomb(H, vd.Y2, vd.Y1, dt / 3, vd.fo);
  tfield(n, w, ws, t0 + dt / 3, v.Y2, v.fo, true);                   // k2
  tfield_tan(n, w, x, ws, vd.Y2, vd.fo);
  tcomb(H, v.Y3, v.Y1, dt, v.fo, -dt / 3, v.cc);
  tcomb(H, vd.Y3, vd.Y1, dt, vd.fo, -dt / 3, vd.cc);
  tcomb(H, v.cc, v.cc, -1.0, v.fo);                                  // cc = k1 - k2
  tcomb(H, vd.cc, vd.cc, -1.0, vd.fo);
  tfield(n, w, ws, t0 + 2 * dt / 3, v.Y3, v.fo, true);               // k3
  tfield_tan(n, w, x, ws, vd.Y3, vd.fo);
  tcomb(H, v.Y4, v.Y1, dt, v.cc, dt, v.fo);
  tcomb(H, vd.Y4, vd.Y1, dt, vd.cc, dt, vd.fo);
  tcomb(H, v.a, nullptr, dt / 8, v.lam);
  tcomb(H, vd.a, nullptr, dt / 8, vd.lam);
  tfield_vjp_tan(n, w, x, ws, t0 + dt, v.Y4, vd.Y4, v.a, vd.a, v.g4, vd.g4);
  tcomb(H, v.a, nullptr, 3 * dt / 8, v.lam, dt, v.g4);
  tcomb(H, vd.a, nullptr, 3 * dt / 8, vd.lam, dt, vd.g4);
  tfield_vjp_tan(n, w, x, ws, t0 + 2 * dt / 3, v.Y3, vd.Y3, v.a, vd.a, v.g3, vd.g3);
  tcomb(H, v.a, nullptr, 3 * dt / 8, v.lam, -dt, v.g4, dt, v.g3);
  tcomb(H, vd.a, nullptr, 3 * dt / 8, vd.lam, -dt, vd.g4, dt, vd.g3);
  tfield_vjp_tan(n, w, x, ws, t0 + dt / 3, v.Y2, vd.Y2, v.a, vd.a, v.g2, vd.g2);
  for (int e = lane_id(); e < 16 * H; e += 64) {
    v.a[e] = (dt / 8) * v.lam[e] + dt * v.g4[e] - (dt / 3) * v.g3[e] + (dt / 3) * v.g2[e];
    vd.a[e] = (dt / 8) * vd.lam[e] + dt * vd.g4[e] - (dt / 3) * vd.g3[e] + (dt / 3) * vd.g2[e];
  }
  sync_tile();
  tfield_vjp_tan(n, w, x, ws, t0, v.Y1, vd.Y1, v.a, vd.a, v.gy, vd.gy);
  for (int e = lane_id(); e < 16 * H; e += 64) {
    v.lam[e] += v.g4[e] + v.g3[e] + v.g2[e] + v.gy[e];
    vd.lam[e] += vd.g4[e] + vd.g3[e] + vd.g2[e] + vd.gy[e];
  }
  sync_tile();
}

__global__ void __launch_bounds__(64) kt_paths_jvp(XwPathsHvpJob job, const double* __restrict__ theta, int method, int L, int d, int H,
                                                    int K, int m, double* __restrict__ work) {
  const int N = job.N, p0 = blockIdx.x * 16;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TileWork w = tile_work(1, d, H, K, m);
  const HvpWork x = hvp_work(w, d, H, K);
  double* ws = work + (long)blockIdx.x * x.total;
  const SweepVecs v = sweep_vecs(ws + w.hv, H), vd = sweep_vecs(ws + x.hvd, H);
  const int l16 = lane_id() & 15;
  const int pc = p0 + l16 < N ? p0 + l16 : N - 1;                 // the lane's own path
  const int ns = tile_steps(job.nstep, N, p0, L);
  hvp_prologue(n, w, x, ws, job, p0);
  // yd_0 = IL4 gate(IL2 gate(IL0_w vs)): the lift's tangent along vs, its gates from the lift itself
  double* yd = vd.lam;
  tlift(n, ws + w.st, v.Y2, v.Y3, v.Y4);
  for (int e = lane_id(); e < 16 * H; e += 64) vd.Y2[e] = v.Y2[e] > 0.0 ? theta[n.o.IL0w + (e >> 4)] * ws[x.vs + (e & 15)] : 0.0;
  sync_tile();
  tgemm(theta + n.o.IL2w, H, 1, H, H, vd.Y2, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, v.Y3, vd.Y3);
  tgemm(theta + n.o.IL4w, H, 1, H, H, vd.Y3, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, yd);
  tstore(H, N, p0, yd, job.Yd);
  for (int l = 1; l <= ns; ++l) {
    tload(H, N, p0, job.Y + (long)(l - 1) * H * N, v.Y1);
    sync_tile();
    const double t0 = job.tT[(long)(l - 1) * N + pc], dt = job.tT[(long)l * N + pc] - t0;
    if (method == 0) {
      tfield(n, w, ws, t0, v.Y1, nullptr, true);
      tfield_tan(n, w, x, ws, yd, vd.fo);
      tcomb(H, yd, yd, dt, vd.fo);
    } else if (method == 1) {
      tfield(n, w, ws, t0, v.Y1, v.fo, true);
      tfield_tan(n, w, x, ws, yd, vd.fo);
      tcomb(H, v.Y2, v.Y1, dt / 2, v.fo);
      tcomb(H, vd.Y2, yd, dt / 2, vd.fo);
      tfield(n, w, ws, t0 + dt / 2, v.Y2, nullptr, true);
      tfield_tan(n, w, x, ws, vd.Y2, vd.fo);
      tcomb(H, yd, yd, dt, vd.fo);
    } else {                                                         // (tstep_rk4's sequence; acc for the tangent alone)
      double* accd = vd.g4;
      tfield(n, w, ws, t0, v.Y1, v.fo, true);                        // k1; cc = k1
      tfield_tan(n, w, x, ws, yd, vd.fo);
      tcomb(H, accd, nullptr, 1.0, vd.fo);
      tcomb(H, v.cc, nullptr, 1.0, v.fo);
      tcomb(H, vd.cc, nullptr, 1.0, vd.fo);
      tcomb(H, v.Y2, v.Y1, dt / 3, v.fo);
      tcomb(H, vd.Y2, yd, dt / 3, vd.fo);
      tfield(n, w, ws, t0 + dt / 3, v.Y2, v.fo, true);               // k2
      tfield_tan(n, w, x, ws, vd.Y2, vd.fo);
      tcomb(H, accd, accd, 3.0, vd.fo);
      tcomb(H, v.Y3, v.Y1, dt, v.fo, -dt / 3, v.cc);
      tcomb(H, vd.Y3, yd, dt, vd.fo, -dt / 3, vd.cc);
      tcomb(H, v.cc, v.cc, -1.0, v.fo);                              // cc = k1 - k2
      tcomb(H, vd.cc, vd.cc, -1.0, vd.fo);
      tfield(n, w, ws, t0 + 2 * dt / 3, v.Y3, v.fo, true);           // k3
      tfield_tan(n, w, x, ws, vd.Y3, vd.fo);
      tcomb(H, accd, accd, 3.0, vd.fo);
      tcomb(H, v.Y4, v.Y1, dt, v.cc, dt, v.fo);
      tcomb(H, vd.Y4, yd, dt, vd.cc, dt, vd.fo);
      tfield(n, w, ws, t0 + dt, v.Y4, nullptr, true);                // k4
      tfield_tan(n, w, x, ws, vd.Y4, vd.fo);
      tcomb(H, accd, accd, 1.0, vd.fo);
      tcomb(H, yd, yd, dt / 8, accd);
    }
    tstore(H, N, p0, yd, job.Yd + (long)l * H * N);
  }
  for (int l = ns + 1; l < L; ++l) tstore(H, N, p0, yd, job.Yd + (long)l * H * N);   // the rows behind the tile's last step
  if (job.ju && lane_id() < 16 && p0 + l16 < N) {
    const double* flw = theta + n.o.FLw;
    double s = 0.0;
    for (int h = 0; h < H; ++h) s = fma(flw[h], yd[h * 16 + l16], s);
    job.ju[p0 + l16] = s;
  }
}

__global__ void __launch_bounds__(64) kt_paths_hvp(XwPathsHvpJob job, const double* __restrict__ theta, int method, int L, int d, int H,
                                                    int K, int m, double* __restrict__ work) {
  const int N = job.N, p0 = blockIdx.x * 16;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TileWork w = tile_work(1, d, H, K, m);
  const HvpWork x = hvp_work(w, d, H, K);
  double* ws = work + (long)blockIdx.x * x.total;
  const SweepVecs v = sweep_vecs(ws + w.hv, H), vd = sweep_vecs(ws + x.hvd, H);
  double* Sx = ws + w.total - 16L * K;
  double* Sxd = ws + x.sxd;
  const int l16 = lane_id() & 15;
  const int pc = p0 + l16 < N ? p0 + l16 : N - 1;                 // the lane's own path
  const double* flw = theta + n.o.FLw;
  const int ns = tile_steps(job.nstep, N, p0, L);
  // prologue: Sx = Sxd = 0, lam = FL_w (the cotangent 1 on u at row ns) and lamd = 0 (FL is linear)
  for (int e = lane_id(); e < 16 * K; e += 64) Sx[e] = 0.0, Sxd[e] = 0.0;
  for (int e = lane_id(); e < 16 * H; e += 64) v.lam[e] = flw[e >> 4], vd.lam[e] = 0.0;
  hvp_prologue(n, w, x, ws, job, p0);
  for (int l = ns; l >= 1; --l) {
    tload(H, N, p0, job.Y + (long)(l - 1) * H * N, v.Y1);
    tload(H, N, p0, job.Yd + (long)(l - 1) * H * N, vd.Y1);
    sync_tile();
    // y_l = step(y_{l-1}): (lam, lamd) become those of y_{l-1}; kt_paths_grad's text, every line with its tangent
    const double t0 = job.tT[(long)(l - 1) * N + pc], dt = job.tT[(long)l * N + pc] - t0;
    if (method == 0) {
      tcomb(H, v.a, nullptr, dt, v.lam);
      tcomb(H, vd.a, nullptr, dt, vd.lam);
      tfield_vjp_tan(n, w, x, ws, t0, v.Y1, vd.Y1, v.a, vd.a, v.gy, vd.gy);
      tcomb(H, v.lam, v.lam, 1.0, v.gy);
      tcomb(H, vd.lam, vd.lam, 1.0, vd.gy);
    } else if (method == 1) {
      tfield(n, w, ws, t0, v.Y1, v.fo, true);
      tfield_tan(n, w, x, ws, vd.Y1, vd.fo);
      tcomb(H, v.Y2, v.Y1, dt / 2, v.fo);
      tcomb(H, vd.Y2, vd.Y1, dt / 2, vd.fo);
      tcomb(H, v.a, nullptr, dt, v.lam);
      tcomb(H, vd.a, nullptr, dt, vd.lam);
      tfield_vjp_tan(n, w, x, ws, t0 + dt / 2, v.Y2, vd.Y2, v.a, vd.a, v.gy, vd.gy);
      tcomb(H, v.lam, v.lam, 1.0, v.gy);
      tcomb(H, vd.lam, vd.lam, 1.0, vd.gy);
      tcomb(H, v.a, nullptr, dt / 2, v.gy);
      tcomb(H, vd.a, nullptr, dt / 2, vd.gy);
      tfield_vjp_tan(n, w, x, ws, t0, v.Y1, vd.Y1, v.a, vd.a, v.gy, vd.gy);
      tcomb(H, v.lam, v.lam, 1.0, v.gy);
      tcomb(H, vd.lam, vd.lam, 1.0, vd.gy);
    } else {
      tstep_rk4_bwd_tan(n, w, x, ws, t0, dt, v, vd);
    }
  }
  // tail: the lift reversed on lamd for hs (its gates from the lift itself), Win[:, :d]^T Sxd for hx
  if (job.hs) {
    double *p0v = v.Y2, *p2v = v.Y3, *y0 = v.Y4, *dh2 = vd.fo, *dh1 = vd.g4;
    tlift(n, ws + w.st, p0v, p2v, y0);
    tgemm(theta + n.o.IL4w, 1, H, H, H, vd.lam, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p2v, dh2);
    tgemm(theta + n.o.IL2w, 1, H, H, H, dh2, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p0v, dh1);
    if (lane_id() < 16 && p0 + l16 < N) {
      double s = 0.0;
      for (int i = 0; i < H; ++i) s = fma(theta[n.o.IL0w + i], dh1[i * 16 + l16], s);
      job.hs[p0 + l16] = s;
    }
  }
  if (job.hx) {
    double* hxt = ws + w.xt + 16L * d;
    tgemm(theta + n.o.Win, 1, n.o.ldin, d, K, Sxd, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, hxt);
    tstore(d, N, p0, hxt, job.hx);
  }
}

}  // namespace

// ---- entry points (include/xnwan_hess.h) ------------------------------------------------------------------------------------------
extern "C" int xw_paths_tiled_hvp_work(int d, int H, int K, int m) {
  if (!xw_tiled_ode_ok(d, H, K, m)) return -1;
  return (int)hvp_work(tile_work(1, d, H, K, m), d, H, K).total;
}

extern "C" int xw_paths_tiled_hvp(const XwPathsHvpJob* jobs, int njobs, const double* theta, int method, int L, int d, int H, int K,
                                  int m, double* work, void* stream) {
  if (!jobs || njobs < 1 || !theta || !work || L < 1 || method < 0 || method > 2) return XW_E_ARG;
  if (!xw_tiled_ode_ok(d, H, K, m)) return XW_E_DIMS;
  for (int i = 0; i < njobs; ++i) {
    const XwPathsHvpJob& j = jobs[i];
    if (!j.xT || !j.start || !j.tT || !j.Y || !j.vx || !j.vs || !j.Yd || !(j.ju || j.hx || j.hs) || j.N < 1) return XW_E_ARG;
  }
  const long per = hvp_work(tile_work(1, d, H, K, m), d, H, K).total;
  long off = 0;
  for (int i = 0; i < njobs; ++i) {
    const int tiles = (jobs[i].N + 15) / 16;
    hipLaunchKernelGGL(kt_paths_jvp, dim3(tiles), dim3(64), 0, (hipStream_t)stream, jobs[i], theta, method, L, d, H, K, m, work + off);
    if (jobs[i].hx || jobs[i].hs)
      hipLaunchKernelGGL(kt_paths_hvp, dim3(tiles), dim3(64), 0, (hipStream_t)stream, jobs[i], theta, method, L, d, H, K, m, work + off);
    off += per * tiles;
  }
  return xw_launch_status();
}
