// xw_tiled_paths.hip -- the tiled stepper's forward pass over a RAGGED group: every path on a time grid of its own.
//
// kt_ode_fwd (xw_tiled.hip) takes one grid t[L] for all paths of a job.  Here path p of a job has its own non-decreasing times
// tT[0 .. L)[p] (time-major, [L][N]); a path with fewer steps than L - 1 repeats its last time, and a zero-length step is the
// exact identity of all three schemes (fma(0, k, y) == y), so its padded rows hold its final value.  One wave per 16-path tile,
// kt_ode_fwd's workspace and its step function (tstep_fwd of xw_tiled_blocks.h, which says why it takes them): t0 and dt live in a
// register per lane -- the lane's own path, column lane & 15.  A job whose paths all carry one grid reproduces kt_ode_fwd to the bit.
//
// nstep[N] (optional): the index of each path's last distinct time.  A tile takes max(nstep) over its real paths as its step count
// and fills the later rows with the state it has, without evaluating the field: the cost of a launch is the sum over tiles of
// max nstep, not N (L - 1).  last_only: only the final row is stored, u[N] (and Y[H][N]).
// Lanes past the end of a job walk with the last path and store nothing.  No float atomics, no waits between blocks.
#include "xw_common.h"
#include "xnwan.h"

namespace {
#include "xw_generic_cot.h"   // (not used by this forward pass: the sweep helpers of xw_tiled_blocks.h name cot_u / cot_job_ok)
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
  for (int l = 0; l < rows; ++l) {
    if (l > 0 && l <= ns) {
      const double t0 = job.tT[(long)(l - 1) * N + pc], dt = job.tT[(long)l * N + pc] - t0;
      tstep_fwd(n, w, ws, method, t0, dt, y, acc, cc, tmp, fo);
    }
    if (job.last_only && l < ns) continue;
    const long row = job.last_only ? 0 : l;                      // (rows past ns: the state the tile has, stored again)
    tput_output(n, job.u, job.Y, row, N, p0, y);
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
