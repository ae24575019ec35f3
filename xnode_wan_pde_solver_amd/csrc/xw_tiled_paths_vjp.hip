// xw_tiled_paths_vjp.hip -- the tiled stepper's reverse sweep over a RAGGED group WITH parameter gradients: every path on a time
// grid of its own, the cotangent w_p on path p's FINAL value (include/xnwan_vjp.h).
//
// It is kt_paths_grad's walk (xw_tiled_paths_grad.hip: one wave per 16-path tile, the checkpoints Y[L][H][N] of kt_ode_fwd_pp read
// back, never recomputed, t0 and dt in a register per lane, ns = min(L - 1, max nstep over the tile's real paths) steps) with two
// differences: lam = w_p FL_w on row ns, not FL_w; and every VJP, the read-out and the lift's reverse add the tile's parameter
// gradients to its slab gslab[tile][P_u], kt_ode_bwd's slab format (xw_tiled.hip), so xw_slab_sum and what follows it are unchanged.
//
// What the shared blocks cannot serve here, restated in xw_tiled_paths_blocks.h (vfield_vjp, VjpWork: shared with
// xw_tiled_paths_gvjp.hip) and below (vstep_rk4_bwd):
//   * tfield_vjp gives the time column of Win one scalar t times the sum of dz over the 16 paths.  Here every path has its own stage
//     time, so the column needs sum_p t_p dz[r][p]: vfield_vjp keeps the 16 stage times in the workspace (VjpWork.tv) and hands them
//     to trowsum as its weights.  vstep_rk4_bwd is tstep_rk4_bwd calling it.
//   * euler's and midpoint's reverse exist in kt_ode_bwd's and kt_paths_grad's own text only.
// Lanes past the end of a job walk with the last path on the weight 0 EXACTLY: lam = 0 FL_w, every stage cotangent is 0 * finite,
// every outer product and row sum adds exact zeros -- the last path is not counted twice.  The same holds for a path with w_p = 0
// and for a zero-length step (dt = 0) of a shorter path: the slab's bits do not move.
// Every slab entry is updated by one fixed lane in program order (touter, trowsum): no float atomics, no waits between blocks, no
// LDS; the same launch twice gives the same bits and the launch can be captured.
#include "xw_common.h"
#include "xnwan_hess.h"       // (xw_tiled_paths_blocks.h names XwPathsHvpJob)
#include "xnwan_vjp.h"

namespace {
#include "xw_generic_cot.h"   // (not used by this sweep: the sweep helpers of xw_tiled_blocks.h name cot_u / cot_job_ok)
#include "xw_tiled_blocks.h"
#include "xw_tiled_paths_blocks.h"   // VjpWork, vfield_vjp (shared with xw_tiled_paths_gvjp.hip)

// tstep_rk4_bwd on vfield_vjp (no further cotangent on k1): v.lam, the cotangent of y_l, becomes that of y_{l-1} (in v.Y1)
__device__ __forceinline__ void vstep_rk4_bwd(const Net& n, const TileWork& w, const VjpWork& x, double* ws, double t0, double dt,
                                              const SweepVecs& v, double* slab) {
  const int H = n.H;
  double *lam = v.lam, *Y1 = v.Y1, *Y2 = v.Y2, *Y3 = v.Y3, *Y4 = v.Y4, *cc = v.cc, *fo = v.fo, *g4 = v.g4, *g3 = v.g3, *g2 = v.g2,
         *a = v.a, *gy = v.gy;
  tfield(n, w, ws, t0, Y1, fo, true);                        // k1; cc = k1
  tcomb(H, cc, nullptr, 1.0, fo);
  tcomb(H, Y2, Y1, dt / 3, fo);
  tfield(n, w, ws, t0 + dt / 3, Y2, fo, true);               // k2
  tcomb(H, Y3, Y1, dt, fo, -dt / 3, cc);
  tcomb(H, cc, cc, -1.0, fo);                                // cc = k1 - k2
  tfield(n, w, ws, t0 + 2 * dt / 3, Y3, fo, true);           // k3
  tcomb(H, Y4, Y1, dt, cc, dt, fo);
  tcomb(H, a, nullptr, dt / 8, lam);
  vfield_vjp(n, w, x, ws, t0 + dt, Y4, a, g4, slab);
  tcomb(H, a, nullptr, 3 * dt / 8, lam, dt, g4);
  vfield_vjp(n, w, x, ws, t0 + 2 * dt / 3, Y3, a, g3, slab);
  tcomb(H, a, nullptr, 3 * dt / 8, lam, -dt, g4, dt, g3);
  vfield_vjp(n, w, x, ws, t0 + dt / 3, Y2, a, g2, slab);
  for (int e = lane_id(); e < 16 * H; e += 64) a[e] = (dt / 8) * lam[e] + dt * g4[e] - (dt / 3) * g3[e] + (dt / 3) * g2[e];
  sync_tile();
  vfield_vjp(n, w, x, ws, t0, Y1, a, gy, slab);
  for (int e = lane_id(); e < 16 * H; e += 64) lam[e] += g4[e] + g3[e] + g2[e] + gy[e];
  sync_tile();
}

__global__ void __launch_bounds__(64) kt_paths_vjp(XwPathsVjpJob job, const double* __restrict__ theta, int method, int L, int d,
                                                    int H, int K, int m, double* __restrict__ work) {
  const int N = job.N, p0 = blockIdx.x * 16;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TileWork w = tile_work(1, d, H, K, m);
  const VjpWork x = vjp_work(w);
  double* ws = work + (long)blockIdx.x * x.total;
  double* slab = job.gslab + (long)blockIdx.x * n.o.total;
  const SweepVecs v = sweep_vecs(ws + w.hv, H);
  double* wv = ws + w.ub;                                          // the weights: the cotangent on u at row ns
  double* st = ws + w.st;
  double* Sx = ws + w.total - 16L * K;
  const int l16 = lane_id() & 15;
  const bool lane_active = p0 + l16 < N;
  const int pc = lane_active ? p0 + l16 : N - 1;                   // the lane's own path
  const double* flw = theta + n.o.FLw;
  int ns = L - 1;                                                  // the tile's step count: the forward's rule
  if (job.nstep) {
    int mx = 0;
    for (int q = 0; q < 16 && p0 + q < N; ++q) mx = job.nstep[p0 + q] > mx ? job.nstep[p0 + q] : mx;
    ns = mx < ns ? mx : ns;
  }
  // prologue: the start values, the weights (exactly 0 past the end of the job), Sx = 0, the tile's x and xproj, y_ns
  if (lane_id() < 16) {
    st[l16] = job.start[pc];
    wv[l16] = lane_active ? job.w[p0 + l16] : 0.0;
  }
  for (int e = lane_id(); e < 16 * K; e += 64) Sx[e] = 0.0;
  tload(H, N, p0, job.Y + (long)ns * H * N, v.Y2);
  tile_x(n, w, ws, job.xT, N, p0);
  // the cotangent w_p on u_p = FL(y_ns): lam = w_p FL_w, the read-out's gradient into the slab
  for (int e = lane_id(); e < 16 * H; e += 64) v.lam[e] = flw[e >> 4] * wv[e & 15];
  readout_grad(slab, n, v.Y2, wv);
  sync_tile();
  for (int l = ns; l >= 1; --l) {
    tload(H, N, p0, job.Y + (long)(l - 1) * H * N, v.Y1);
    sync_tile();
    // y_l = step(y_{l-1}): lam becomes the cotangent of y_{l-1}
    const double t0 = job.tT[(long)(l - 1) * N + pc], dt = job.tT[(long)l * N + pc] - t0;
    if (method == 0) {
      tcomb(H, v.a, nullptr, dt, v.lam);
      vfield_vjp(n, w, x, ws, t0, v.Y1, v.a, v.gy, slab);
      tcomb(H, v.lam, v.lam, 1.0, v.gy);
    } else if (method == 1) {
      tfield(n, w, ws, t0, v.Y1, v.fo, true);
      tcomb(H, v.Y2, v.Y1, dt / 2, v.fo);
      tcomb(H, v.a, nullptr, dt, v.lam);
      vfield_vjp(n, w, x, ws, t0 + dt / 2, v.Y2, v.a, v.gy, slab);
      tcomb(H, v.lam, v.lam, 1.0, v.gy);
      tcomb(H, v.a, nullptr, dt / 2, v.gy);
      vfield_vjp(n, w, x, ws, t0, v.Y1, v.a, v.gy, slab);
      tcomb(H, v.lam, v.lam, 1.0, v.gy);
    } else {
      vstep_rk4_bwd(n, w, x, ws, t0, dt, v, slab);
    }
  }
  // tail: the lift 1 -> H -> H -> H reversed, the x columns and the bias of the input layer.  lam is the whole cotangent of y_0: the
  // steps' share, and with ns == 0 the read-out's own (set above) -- sweep_tail's parameter pass with its read-out cotangent folded in
  double *p0v = v.Y2, *p2v = v.Y3, *y0 = v.Y4, *dh2 = v.fo, *dh1 = v.g4;
  tlift(n, st, p0v, p2v, y0);
  tgemm(theta + n.o.IL4w, 1, H, H, H, v.lam, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p2v, dh2);
  tgemm(theta + n.o.IL2w, 1, H, H, H, dh2, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p0v, dh1);
  touter(slab, n.o.IL4w, H, H, H, v.lam, p2v, A_RELU);
  touter(slab, n.o.IL2w, H, H, H, dh2, p0v, A_RELU);
  trowsum(slab, n.o.IL4b, 1, H, v.lam, nullptr, 1.0);
  trowsum(slab, n.o.IL2b, 1, H, dh2, nullptr, 1.0);
  trowsum(slab, n.o.IL0w, 1, H, dh1, st, 1.0);
  trowsum(slab, n.o.IL0b, 1, H, dh1, nullptr, 1.0);
  if (job.gs && lane_id() < 16 && lane_active) {
    double s = 0.0;
    for (int i = 0; i < H; ++i) s = fma(theta[n.o.IL0w + i], dh1[i * 16 + l16], s);
    job.gs[p0 + l16] = s;
  }
  trowsum(slab, n.o.Winb, 1, K, Sx, nullptr, 1.0);
  touter(slab, n.o.Win, n.o.ldin, K, d, Sx, ws + w.xt, A_PLAIN);
  if (job.gx) {
    double* gxt = ws + w.xt + 16L * d;
    tgemm(theta + n.o.Win, 1, n.o.ldin, d, K, Sx, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, gxt);
    tstore(d, N, p0, gxt, job.gx);
  }
}

}  // namespace

// ---- entry points (include/xnwan_vjp.h) -------------------------------------------------------------------------------------------
extern "C" int xw_paths_tiled_vjp_work(int d, int H, int K, int m) {
  if (!xw_tiled_ode_ok(d, H, K, m)) return -1;
  return (int)vjp_work(tile_work(1, d, H, K, m)).total;
}

extern "C" int xw_paths_tiled_vjp(const XwPathsVjpJob* jobs, int njobs, const double* theta, int method, int L, int d, int H, int K,
                                  int m, double* work, void* stream) {
  if (!jobs || njobs < 1 || !theta || !work || L < 1 || method < 0 || method > 2) return XW_E_ARG;
  if (!xw_tiled_ode_ok(d, H, K, m)) return XW_E_DIMS;
  for (int i = 0; i < njobs; ++i) {
    const XwPathsVjpJob& j = jobs[i];
    if (!j.xT || !j.start || !j.tT || !j.Y || !j.w || !j.gslab || j.N < 1) return XW_E_ARG;
  }
  const long per = vjp_work(tile_work(1, d, H, K, m)).total, P = u_offsets(d, H, K).total;
  long off = 0;
  for (int i = 0; i < njobs; ++i) {
    const int tiles = (jobs[i].N + 15) / 16;
    const hipError_t e = hipMemsetAsync(jobs[i].gslab, 0, sizeof(double) * P * tiles, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kt_paths_vjp, dim3(tiles), dim3(64), 0, (hipStream_t)stream, jobs[i], theta, method, L, d, H, K, m, work + off);
    off += per * tiles;
  }
  return xw_launch_status();
}
