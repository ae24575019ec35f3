// xw_tiled_paths_blocks.h -- what the per-path sweeps with parameter gradients and with tangents share: the workspaces behind the
// tile's TileWork (VjpWork: the 16 stage times; HvpWork: the tangent vectors), the field's VJP with a stage time per path and a slab
// (vfield_vjp), the field's tangent and the tangent of its VJP (tfield_tan, tfield_vjp_tan), the tile's step count and the prologue
// of the direction (tile_steps, hvp_prologue).  Used by xw_tiled_paths_vjp.hip, xw_tiled_paths_hvp.hip and xw_tiled_paths_gvjp.hip.
// Library-internal; included INSIDE an anonymous namespace, after xw_tiled_blocks.h and include/xnwan_hess.h (XwPathsHvpJob).
#pragma once

// behind the tile's TileWork: the stage times of the 16 paths (the weights w_p live in TileWork.ub, the cotangent on u)
struct VjpWork {
  long tv, total;
};
__host__ __device__ inline VjpWork vjp_work(const TileWork& w) {
  VjpWork x;
  x.tv = w.total;
  x.total = w.total + 16;
  return x;
}

// tfield_vjp with a stage time PER PATH (t: the lane's own path's, column lane & 15) and a slab: a^T dF/d(y, theta) at (t, yin) --
// gy (overwritten), Sx += cotangent of z_0, parameter gradients into slab.  tfield_vjp's operations in tfield_vjp's order; the time
// column of Win takes sum_p tv[p] dz[r][p]
__device__ void vfield_vjp(const Net& n, const TileWork& w, const VjpWork& x, double* ws, double t, const double* yin, const double* a,
                           double* gy, double* slab) {
  const int K = n.K, H = n.H, ld = n.o.ldin;
  const double* th = n.th;
  double* tv = ws + x.tv;
  if (lane_id() < 16) tv[lane_id()] = t;                         // (ordered before its reader by tfield's sync_tile)
  tfield(n, w, ws, t, yin, nullptr, true);
  const double* zs = ws + w.zs;
  const double* tz = ws + w.th;
  double* dz = ws + w.dz;
  double* dzp = ws + w.dzp;
  double* Sx = ws + w.total - 16L * K;
  // dz = (Wo^T a) (1 - tanh^2)
  tgemm(th + n.o.Wo, 1, K, K, H, a, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_TANH_D, tz, dz);
  touter(slab, n.o.Wo, K, H, K, a, tz, A_PLAIN);
  trowsum(slab, n.o.Wob, 1, H, a, nullptr, 1.0);
  for (int l = n.m - 1; l >= 1; --l) {
    const double* zp = zs + 16L * K * (l - 1);
    touter(slab, n.o.Wh, K, K, K, dz, zp, A_RELU);
    trowsum(slab, n.o.Whb, 1, K, dz, nullptr, 1.0);
    tgemm(th + n.o.Wh, 1, K, K, K, dz, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, zp, dzp);
    double* s_ = dz; dz = dzp; dzp = s_;
  }
  touter(slab, (long)n.o.Win + n.d + 1, ld, K, H, dz, yin, A_PLAIN);
  trowsum(slab, (long)n.o.Win + n.d, ld, K, dz, tv, 1.0);
  for (int e = lane_id(); e < 16 * K; e += 64) Sx[e] += dz[e];
  // gy = Win[:, d+1:]^T dz
  tgemm(th + n.o.Win + n.d + 1, 1, ld, H, K, dz, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, gy);
}

// ---- the workspace: the sweep's, then the tangents (offsets in doubles from the tile's base) ----------------------------------------
struct HvpWork {
  long vxt, vxp, zd, thd, q, dzd, dzpd, sxd, hvd, vs, total;
};
__host__ __device__ inline HvpWork hvp_work(const TileWork& w, int d, int H, int K) {
  HvpWork x;
  long p = w.total;
  x.vxt = p; p += 16L * d;                            // vx of the 16 paths
  x.vxp = p; p += 16L * K;                            // Win[:, 0..d) vx (no bias): the direction's share of every zd_0
  x.zd = p; p += 32L * K;                             // tangent pre-activations, gated, two in turn
  x.thd = p; p += 16L * K;                            // (1 - tz^2) zd_{m-1}: the tangent of tanh(z_{m-1})
  x.q = p; p += 16L * K;                              // Wo^T a
  x.dzd = p; p += 16L * K;                            // tangents of the pre-activations' cotangents, ...
  x.dzpd = p; p += 16L * K;                           //   ... of the layer below
  x.sxd = p; p += 16L * K;                            // tangent of Sx
  x.hvd = p; p += 16L * H * 12;                       // the tangents of the sweep's twelve H-vectors
  x.vs = p; p += 16;                                  // vs of the 16 paths
  x.total = p;
  return x;
}

// fod = dF(t, yin) . (yd, vx) for the tile, behind tfield(.., zs_all = true) at (t, yin), whose z_l and tanh(z_{m-1}) it reads:
// zd_0 = Win[:, d+1:] yd + vxp, zd_l = Wh gate(zd_{l-1}), thd = (1 - tz^2) zd_{m-1} (with m == 1: of zd_0 itself), fod = Wo thd
// (fod null: thd only).  Every gate is an epilogue of the product that feeds it.
__device__ void tfield_tan(const Net& n, const TileWork& w, const HvpWork& x, double* ws, const double* yd, double* fod) {
  const int K = n.K, H = n.H, ld = n.o.ldin;
  const double* th = n.th;
  const double* zs = ws + w.zs;
  const double* tz = ws + w.th;
  double* thd = ws + x.thd;
  const double* in = yd;
  for (int l = 0; l < n.m; ++l) {
    const bool top = l == n.m - 1;
    double* out = top ? thd : ws + x.zd + 16L * K * (l & 1);
    const int eop = top ? E_TANH_D : E_GATE;
    const double* aux = top ? tz : zs + 16L * K * l;
    if (l == 0) tgemm(th + n.o.Win + n.d + 1, ld, 1, K, H, in, A_PLAIN, nullptr, nullptr, 0, 0.0, ws + x.vxp, eop, aux, out);
    else tgemm(th + n.o.Wh, K, 1, K, K, in, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, eop, aux, out);
    in = out;
  }
  if (fod) tgemm(th + n.o.Wo, K, 1, H, K, thd, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, fod);
}

// tfield_vjp for (a, ad) at (t, yin) with the tangent yind of yin: gy and Sx as tfield_vjp leaves them, and their tangents
// gyd (overwritten) and Sxd += dzd_0.  Top: dzd = (Wo^T ad) (1 - tz^2) - 2 (Wo^T a) tz thd; below: the gates alone.
__device__ void tfield_vjp_tan(const Net& n, const TileWork& w, const HvpWork& x, double* ws, double t, const double* yin,
                               const double* yind, const double* a, const double* ad, double* gy, double* gyd) {
  const int K = n.K, H = n.H, ld = n.o.ldin;
  const double* th = n.th;
  tfield_vjp(n, w, ws, t, yin, a, gy, nullptr);                      // (leaves every z_l and tz of (t, yin) behind)
  tfield_tan(n, w, x, ws, yind, nullptr);
  const double* zs = ws + w.zs;
  const double* tz = ws + w.th;
  const double* thd = ws + x.thd;
  double* q = ws + x.q;
  double* dzd = ws + x.dzd;
  double* dzpd = ws + x.dzpd;
  double* Sxd = ws + x.sxd;
  tgemm(th + n.o.Wo, 1, K, K, H, a, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, q);
  tgemm(th + n.o.Wo, 1, K, K, H, ad, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_TANH_D, tz, dzd);
  for (int e = lane_id(); e < 16 * K; e += 64) dzd[e] -= 2.0 * q[e] * tz[e] * thd[e];
  sync_tile();
  for (int l = n.m - 1; l >= 1; --l) {
    tgemm(th + n.o.Wh, 1, K, K, K, dzd, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, zs + 16L * K * (l - 1), dzpd);
    double* s_ = dzd; dzd = dzpd; dzpd = s_;
  }
  for (int e = lane_id(); e < 16 * K; e += 64) Sxd[e] += dzd[e];
  tgemm(th + n.o.Win + n.d + 1, 1, ld, H, K, dzd, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, gyd);
}

// the tile's step count (the forward's rule) and, for both kernels, the start values, the direction, x, xproj and vxp
__device__ __forceinline__ int tile_steps(const int* nstep, int N, int p0, int L) {
  int ns = L - 1;
  if (nstep) {
    int mx = 0;
    for (int q = 0; q < 16 && p0 + q < N; ++q) mx = nstep[p0 + q] > mx ? nstep[p0 + q] : mx;
    ns = mx < ns ? mx : ns;
  }
  return ns;
}
__device__ __forceinline__ void hvp_prologue(const Net& n, const TileWork& w, const HvpWork& x, double* ws, const XwPathsHvpJob& job,
                                             int p0) {
  const int N = job.N, l16 = lane_id() & 15;
  const int pc = p0 + l16 < N ? p0 + l16 : N - 1;
  if (lane_id() < 16) {
    ws[w.st + l16] = job.start[pc];
    ws[x.vs + l16] = job.vs[pc];
  }
  tload(n.d, N, p0, job.vx, ws + x.vxt);
  tile_x(n, w, ws, job.xT, N, p0);                                   // (its sync_tile orders the loads above as well)
  tgemm(n.th + n.o.Win, n.o.ldin, 1, n.K, n.d, ws + x.vxt, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, ws + x.vxp);
}
