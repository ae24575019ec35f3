// xw_tiled_paths_grad.hip -- the tiled stepper's reverse sweep over a RAGGED group: every path on a time grid of its own, the
// cotangent 1 on every path's FINAL value (include/xnwan_grad.h).
//
// kt_ode_fwd_pp (xw_tiled_paths.hip, not last_only) has written the checkpoints Y[L][H][N] of the job; this kernel never recomputes
// the forward.  One wave per 16-path tile, the workspace of a tiled sweep (tile_work(1, ...)), t0 and dt in a register per lane --
// the lane's own path, column lane & 15 -- which the blocks of xw_tiled_blocks.h take as they take a tile-wide scalar (see "one
// step of the fixed-grid schemes" there).  The tile walks ns = min(L - 1, max nstep over its real paths) steps back, the forward's
// count.  The forward holds a path's final state through its padded rows, so the cotangent on the final value is a cotangent on
// row ns of the tile: lam = FL_w there and nothing on any other row.  A zero-length step is the exact identity of the reverse as
// it is of the forward -- every stage cotangent is 0 * lam, every vjp adds exact zeros to lam and to Sx -- so a shorter path is not
// touched by the rounds its neighbours still walk, and a path's bits do not depend on the paths beside it.
//
// Outputs per path p (each may be NULL): gx[d][N] = du_p/dx_p and gs[N] = du_p/dstart_p -- the DISCRETE adjoint: the exact reverse
// of the steps taken, the start value and the grid held fixed, step sizes constants -- and ut[N] = FL_w . F(t_p, x_p, y(t_p)), the
// time derivative of the CONTINUOUS model y' = F, u = FL y at fixed x (not the derivative of the discrete u with respect to the end
// of its grid, which would need d(step)/d(dt)).
// euler's and midpoint's reverse exist in kt_ode_bwd's own text only (xw_tiled.hip says why it keeps one); they are written out here,
// rk4's is tstep_rk4_bwd.  No parameter gradients (slab == nullptr throughout).
// Lanes past the end of a job walk with the last path and store nothing.  No float atomics, no waits between blocks.
#include "xw_common.h"
#include "xnwan_grad.h"

namespace {
#include "xw_generic_cot.h"   // (not used by this sweep: the sweep helpers of xw_tiled_blocks.h name cot_u / cot_job_ok)
#include "xw_tiled_blocks.h"

__global__ void __launch_bounds__(64) kt_paths_grad(XwPathsGradJob job, const double* __restrict__ theta, int method, int L, int d,
                                                     int H, int K, int m, double* __restrict__ work) {
  const int N = job.N, p0 = blockIdx.x * 16;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TileWork w = tile_work(1, d, H, K, m);
  double* ws = work + (long)blockIdx.x * w.total;
  const SweepVecs v = sweep_vecs(ws + w.hv, H);
  double* st = ws + w.st;
  double* Sx = ws + w.total - 16L * K;
  const int l16 = lane_id() & 15;
  const int pc = p0 + l16 < N ? p0 + l16 : N - 1;                 // the lane's own path
  const double* flw = theta + n.o.FLw;
  int ns = L - 1;                                                  // the tile's step count: the forward's rule
  if (job.nstep) {
    int mx = 0;
    for (int q = 0; q < 16 && p0 + q < N; ++q) mx = job.nstep[p0 + q] > mx ? job.nstep[p0 + q] : mx;
    ns = mx < ns ? mx : ns;
  }
  // prologue: the start values, Sx = 0, lam = FL_w (the cotangent 1 on u at row ns), the tile's x and xproj
  if (lane_id() < 16) st[l16] = job.start[pc];
  for (int e = lane_id(); e < 16 * K; e += 64) Sx[e] = 0.0;
  for (int e = lane_id(); e < 16 * H; e += 64) v.lam[e] = flw[e >> 4];
  tile_x(n, w, ws, job.xT, N, p0);
  if (job.ut) {                                                    // ut = FL_w . F(t_end, x, y_final)
    tload(H, N, p0, job.Y + (long)ns * H * N, v.Y1);
    sync_tile();
    tfield(n, w, ws, job.tT[(long)ns * N + pc], v.Y1, v.fo, false);
    if (lane_id() < 16 && p0 + l16 < N) {
      double s = 0.0;
      for (int h = 0; h < H; ++h) s = fma(flw[h], v.fo[h * 16 + l16], s);
      job.ut[p0 + l16] = s;
    }
    sync_tile();
  }
  if (job.gx || job.gs) {
    for (int l = ns; l >= 1; --l) {
      tload(H, N, p0, job.Y + (long)(l - 1) * H * N, v.Y1);
      sync_tile();
      // y_l = step(y_{l-1}): lam becomes the cotangent of y_{l-1}
      const double t0 = job.tT[(long)(l - 1) * N + pc], dt = job.tT[(long)l * N + pc] - t0;
      if (method == 0) {
        tcomb(H, v.a, nullptr, dt, v.lam);
        tfield_vjp(n, w, ws, t0, v.Y1, v.a, v.gy, nullptr);
        tcomb(H, v.lam, v.lam, 1.0, v.gy);
      } else if (method == 1) {
        tfield(n, w, ws, t0, v.Y1, v.fo, true);
        tcomb(H, v.Y2, v.Y1, dt / 2, v.fo);
        tcomb(H, v.a, nullptr, dt, v.lam);
        tfield_vjp(n, w, ws, t0 + dt / 2, v.Y2, v.a, v.gy, nullptr);
        tcomb(H, v.lam, v.lam, 1.0, v.gy);
        tcomb(H, v.a, nullptr, dt / 2, v.gy);
        tfield_vjp(n, w, ws, t0, v.Y1, v.a, v.gy, nullptr);
        tcomb(H, v.lam, v.lam, 1.0, v.gy);
      } else {
        tstep_rk4_bwd(n, w, ws, t0, dt, v, nullptr, nullptr);
      }
    }
    // tail: the lift 1 -> H -> H -> H reversed for gs, Win^T Sx for gx.  lam is the whole cotangent of y_0: the steps' share, and
    // with ns == 0 the read-out's own (FL_w, set above) -- sweep_tail's x side with its read-out cotangent already folded in
    double *p0v = v.Y2, *p2v = v.Y3, *y0 = v.Y4, *dh2 = v.fo, *dh1 = v.g4;
    if (job.gs) {
      tlift(n, st, p0v, p2v, y0);
      tgemm(theta + n.o.IL4w, 1, H, H, H, v.lam, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p2v, dh2);
      tgemm(theta + n.o.IL2w, 1, H, H, H, dh2, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p0v, dh1);
      if (lane_id() < 16 && p0 + l16 < N) {
        double s = 0.0;
        for (int i = 0; i < H; ++i) s = fma(theta[n.o.IL0w + i], dh1[i * 16 + l16], s);
        job.gs[p0 + l16] = s;
      }
    }
    if (job.gx) {
      double* gxt = ws + w.xt + 16L * d;
      tgemm(theta + n.o.Win, 1, n.o.ldin, d, K, Sx, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, gxt);
      tstore(d, N, p0, gxt, job.gx);
    }
  }
}

}  // namespace

// ---- entry points (include/xnwan_grad.h) ------------------------------------------------------------------------------------------
extern "C" int xw_paths_tiled_grad_work(int d, int H, int K, int m) { return xw_tiled_ode_work(1, d, H, K, m); }

extern "C" int xw_paths_tiled_grad(const XwPathsGradJob* jobs, int njobs, const double* theta, int method, int L, int d, int H, int K,
                                   int m, double* work, void* stream) {
  if (!jobs || njobs < 1 || !theta || !work || L < 1 || method < 0 || method > 2) return XW_E_ARG;
  if (!xw_tiled_ode_ok(d, H, K, m)) return XW_E_DIMS;
  for (int i = 0; i < njobs; ++i) {
    const XwPathsGradJob& j = jobs[i];
    if (!j.xT || !j.start || !j.tT || !j.Y || !(j.gx || j.gs || j.ut) || j.N < 1) return XW_E_ARG;
  }
  const long per = tile_work(1, d, H, K, m).total;
  long off = 0;
  for (int i = 0; i < njobs; ++i) {
    const int tiles = (jobs[i].N + 15) / 16;
    hipLaunchKernelGGL(kt_paths_grad, dim3(tiles), dim3(64), 0, (hipStream_t)stream, jobs[i], theta, method, L, d, H, K, m, work + off);
    off += per * tiles;
  }
  return xw_launch_status();
}
