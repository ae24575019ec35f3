// xw_tdopri_blocks.h -- what the kernels of solver 'dopri5' on the tiled stepper family share: the per-tile workspace (the family's
// TileWork, then the stages) and the input of a stage.  Used by xw_tdopri.hip (one step size per job) and xw_tdopri_paths.hip (one
// per path).  Library-internal; included INSIDE an anonymous namespace, after xw_tiled_blocks.h and xw_dopri_ctl.h (DP_A).
#pragma once

// the per-tile workspace: the family's TileWork, then the stages k_0 .. k_6 (sweep: and their cotangents) as H-vectors
struct TdWork {
  TileWork w;
  long k, total;
};
__host__ __device__ inline TdWork td_work(int sweep, int d, int H, int K, int m) {
  TdWork q;
  q.w = tile_work(sweep, d, H, K, m);
  q.k = q.w.total;
  q.total = q.w.total + 16L * H * (sweep ? 14 : 7);
  return q;
}

// a = y + dt sum_{q < st} a_{st,q} k_q: the input of stage st (st = 0: y itself).  dt is passed BY VALUE: the job's (kq_attempt,
// kq_sweep: wave-uniform) or the lane's own path's (kq_paths) -- the loop touches columns e & 15 == lane & 15 only
__device__ void stage_input(int H, int st, double dt, const double* y, const double* kk, double* a) {
  double c[6];
  for (int q = 0; q < st; ++q) c[q] = DP_A[st][q] * dt;
  for (int e = lane_id(); e < 16 * H; e += 64) {
    double acc = 0.0;
    for (int q = 0; q < st; ++q) acc = fma(kk[16L * H * q + e], c[q], acc);
    a[e] = y[e] + acc;
  }
  sync_tile();
}
