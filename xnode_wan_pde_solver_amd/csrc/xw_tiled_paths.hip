// xw_tiled_paths.hip -- the tiled stepper's forward pass over a RAGGED group: every path on a time grid of its own.
//
// kt_ode_fwd (xw_tiled.hip) takes one grid t[L] for all paths of a job.  Here path p of a job has its own non-decreasing times
// tT[0 .. L)[p] (time-major, [L][N]); a path with fewer steps than L - 1 repeats its last time, and a zero-length step is the
// exact identity of all three schemes (fma(0, k, y) == y), so its padded rows hold its final value.  One wave per 16-path tile,
// kt_ode_fwd's workspace and stage sequences; t0 and dt live in a register per lane -- the lane's own path, column lane & 15 --
// and reach the field's time term and the combinations through the per-path siblings of xw_tiled_blocks.h.  A job whose paths all
// carry one grid reproduces kt_ode_fwd to the bit.
//
// nstep[N] (optional): the index of each path's last distinct time.  A tile takes max(nstep) over its real paths as its step count
// and fills the later rows with the state it has, without evaluating the field: the cost of a launch is the sum over tiles of
// max nstep, not N (L - 1).  last_only: only the final row is stored, u[N] (and Y[H][N]).
// Lanes past the end of a job walk with the last path and store nothing.  No float atomics, no waits between blocks.
#include "xw_common.h"
#include "xnwan.h"

namespace {
#include "xw_tiled_blocks.h"

__global__ void __launch_bounds__(64) kt_ode_fwd_pp(XwPathsJob job, const double* __restrict__ theta, int method, int L, int d, int H,
                                                     int K, int m, double* __restrict__ work) {
  const int N = job.N, p0 = blockIdx.x * 16;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TileWork w = tile_work(0, d, H, K, m);
  double* ws = work + (long)blockIdx.x * w.total;
  double* y = ws + w.hv;
  double* acc = y + 16L * H;
  double* cc = acc + 16L * H;
  double* tmp = cc + 16L * H;
  double* fo = tmp + 16L * H;
  double* st = ws + w.st;
  const int l16 = lane_id() & 15;
  const int pc = p0 + l16 < N ? p0 + l16 : N - 1;                 // the lane's own path
  if (lane_id() < 16) st[l16] = job.start[pc];
  tile_x(n, w, ws, job.xT, N, p0);
  tlift(n, st, acc, cc, y);
  int ns = L - 1;                                                  // the tile's step count
  if (job.nstep) {
    int mx = 0;
    for (int q = 0; q < 16 && p0 + q < N; ++q) mx = job.nstep[p0 + q] > mx ? job.nstep[p0 + q] : mx;
    ns = mx < ns ? mx : ns;
  }
  const int rows = job.last_only ? ns + 1 : L;
  const double* flw = theta + n.o.FLw;
  for (int l = 0; l < rows; ++l) {
    if (l > 0 && l <= ns) {
      const double t0 = job.tT[(long)(l - 1) * N + pc], dt = job.tT[(long)l * N + pc] - t0;
      if (method == 0) {
        tfield_pp(n, w, ws, t0, y, fo);
        tcomb_pp(H, y, y, dt, fo);
      } else if (method == 1) {
        tfield_pp(n, w, ws, t0, y, fo);
        tcomb_pp(H, tmp, y, dt / 2, fo);
        tfield_pp(n, w, ws, t0 + dt / 2, tmp, fo);
        tcomb_pp(H, y, y, dt, fo);
      } else {                                                   // 3/8 rule: acc = k1 + 3 k2 + 3 k3 + k4, cc = k1 - k2
        tfield_pp(n, w, ws, t0, y, fo);
        tcomb_pp(H, acc, nullptr, 1.0, fo);
        tcomb_pp(H, cc, nullptr, 1.0, fo);
        tcomb_pp(H, tmp, y, dt / 3, fo);
        tfield_pp(n, w, ws, t0 + dt / 3, tmp, fo);
        tcomb_pp(H, acc, acc, 3.0, fo);
        tcomb_pp(H, tmp, y, dt, fo, -dt / 3, cc);
        tcomb_pp(H, cc, cc, -1.0, fo);
        tfield_pp(n, w, ws, t0 + 2 * dt / 3, tmp, fo);
        tcomb_pp(H, acc, acc, 3.0, fo);
        tcomb_pp(H, tmp, y, dt, cc, dt, fo);
        tfield_pp(n, w, ws, t0 + dt, tmp, fo);
        tcomb_pp(H, acc, acc, 1.0, fo);
        tcomb_pp(H, y, y, dt / 8, acc);
      }
    }
    if (job.last_only && l < ns) continue;
    const long row = job.last_only ? 0 : l;                      // (rows past ns: the state the tile has, stored again)
    if (lane_id() < 16 && p0 + l16 < N) {
      double u = theta[n.o.FLb];
      for (int j = 0; j < H; ++j) u = fma(flw[j], y[j * 16 + l16], u);
      job.u[row * N + p0 + l16] = u;
    }
    if (job.Y)
      for (int e = lane_id(); e < 16 * H; e += 64)
        if (p0 + (e & 15) < N) job.Y[(row * H + (e >> 4)) * N + p0 + (e & 15)] = y[e];
  }
}

}  // namespace

// ---- entry points (include/xnwan.h) -------------------------------------------------------------------------------------------
extern "C" int xw_paths_tiled_work(int d, int H, int K, int m) { return xw_tiled_ode_work(0, d, H, K, m); }

extern "C" int xw_paths_tiled_fwd(const XwPathsJob* jobs, int njobs, const double* theta, int method, int L, int d, int H, int K, int m,
                                  double* work, void* stream) {
  if (!jobs || njobs < 1 || !theta || !work || L < 1 || method < 0 || method > 2) return XW_E_ARG;
  if (!xw_tiled_ode_ok(d, H, K, m)) return XW_E_DIMS;
  for (int i = 0; i < njobs; ++i)
    if (!jobs[i].xT || !jobs[i].start || !jobs[i].tT || !jobs[i].u || jobs[i].N < 1) return XW_E_ARG;
  const long per = tile_work(0, d, H, K, m).total;
  long off = 0;
  for (int i = 0; i < njobs; ++i) {
    const int tiles = (jobs[i].N + 15) / 16;
    hipLaunchKernelGGL(kt_ode_fwd_pp, dim3(tiles), dim3(64), 0, (hipStream_t)stream, jobs[i], theta, method, L, d, H, K, m, work + off);
    off += per * tiles;
  }
  return xw_launch_status();
}
