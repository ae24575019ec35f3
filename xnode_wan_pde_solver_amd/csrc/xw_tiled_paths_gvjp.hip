// xw_tiled_paths_gvjp.hip -- PARAMETER gradients of u, of du/d(x, s) along a direction and of ut over a RAGGED group: the tangent of
// kt_paths_vjp's slab-writing sweep (xw_tiled_paths_vjp.hip) along a direction (vx_p, vs_p) per path, with one term at the top of
// the sweep for ut (include/xnwan_grad_vjp.h):
//   J = sum_p [ wu_p U_p + (dU_p/dx . vx_p + dU_p/ds vs_p) + wt_p FL_w . F(t_p, x_p, y_{n_p}) ],   gslab = the tiles' shares of dJ/dtheta.
//
// d/dtheta of the directional derivative is the directional derivative of dU/dtheta: kt_paths_hvp's walk (xw_tiled_paths_hvp.hip:
// lam and Sx recomputed, their tangents lamd and Sxd beside them, Y and Yd read back, never recomputed -- Yd is what kt_paths_jvp
// wrote; the CALLER runs xw_paths_tiled_hvp with ju alone before this launch) with every slab update of kt_paths_vjp replaced by its
// tangent: where that sweep adds outer(dz, a), this one adds outer(dzd, a) + outer(dz, ad) -- dzd from tfield_vjp_tan's chain, its
// -2 (Wo^T a) tz thd term included, ad the tangent of the layer's input: the gated zd_l, thd, yd, vx for Win's x columns, 0 for its
// time column.  The lift and the hidden layers are ReLU, so the tanh term is the one curvature.
// The chain (lamd, dzd, Sxd) is LINEAR in its start: lamd on row ns is wu_p FL_w + wt_p (dF/dy)^T FL_w, not 0, and the outer
// products of dzd carry the shares of wu and wt as well.  The top of the sweep: one tangent VJP of F at (t_p, x_p, y_ns) with a = 0
// and ad = wt_p FL_w -- the field's own parameters under ut, and (dF/dy)^T FL_w in gyd --, then the read-out's
// FL_w += wu y_ns + yd_ns + wt F and FL_b += wu.  The primal chain lam keeps the weight 1 on every lane.
//
// What the shared blocks cannot serve here, restated below:
//   * tfield_tan keeps two gated tangents in turn; the slab needs the input tangent of EVERY hidden layer while the chain walks
//     down, so gfield_tan keeps them all (GvjpWork.zda), tfield's zs_all for the tangent.  tfield_tan serves the stages that are
//     only recomputed.
//   * tfield_vjp_tan writes no slab and takes one time; gfield_vjp_tan is its text with the slab updates of vfield_vjp, each with
//     its tangent, and vfield_vjp's stage time per path (GvjpWork.tv) for Win's time column.
//   * hvp_prologue hands lanes past the end of a job the last path's direction: harmless where nothing is summed over the paths, a
//     path counted twice here.  This prologue gives them -- and every path of a job without a direction -- exact zeros, and Yd is
//     loaded the same way (tload0).
// Lanes past the end of a job carry wu = wt = 0 and a zero direction EXACTLY: yd, thd, every zd, lamd, dzd, Sxd and the lift's
// tangents are exact zeros there, so every outer product and row sum adds exact zeros -- the same holds for a path whose weights and
// direction are zero, and a zero-length step (dt = 0) is the exact identity for (lam, lamd, Sx, Sxd) and moves no slab bit.
// Every slab entry is updated by one fixed lane in program order (touter, trowsum): no float atomics, no waits between blocks, no
// LDS, no read-back; the same launch twice gives the same bits and the launch can be captured.
#include "xw_common.h"
#include "xnwan_grad_vjp.h"

namespace {
#include "xw_generic_cot.h"   // (not used by this sweep: the sweep helpers of xw_tiled_blocks.h name cot_u / cot_job_ok)
#include "xw_tiled_blocks.h"
#include "xw_tiled_paths_blocks.h"

// behind the tile's HvpWork: the stage times and the weights wt of the 16 paths (wu lives in TileWork.ub), the gated tangent of
// every layer's pre-activation
struct GvjpWork {
  long tv, wt, zda, total;
};
__host__ __device__ inline GvjpWork gvjp_work(const HvpWork& x, int K, int m) {
  GvjpWork g;
  long p = x.total;
  g.tv = p; p += 16;
  g.wt = p; p += 16;
  g.zda = p; p += 16L * K * m;
  g.total = p;
  return g;
}

// tload with exact zeros for the lanes past the end of the job, and everywhere when src is null
__device__ __forceinline__ void tload0(int H, int N, int p0, const double* __restrict__ src, double* v) {
  for (int e = lane_id(); e < 16 * H; e += 64) {
    const int p = p0 + (e & 15);
    v[e] = (src && p < N) ? src[(long)(e >> 4) * N + p] : 0.0;
  }
}

// tfield_tan with every layer kept: the gated zd_l at zda + 16 K l for l < m - 1, thd = (1 - tz^2) zd_{m-1}
__device__ void gfield_tan(const Net& n, const TileWork& w, const HvpWork& x, const GvjpWork& g, double* ws, const double* yd) {
  const int K = n.K, H = n.H, ld = n.o.ldin;
  const double* th = n.th;
  const double* zs = ws + w.zs;
  const double* tz = ws + w.th;
  double* thd = ws + x.thd;
  const double* in = yd;
  for (int l = 0; l < n.m; ++l) {
    const bool top = l == n.m - 1;
    double* out = top ? thd : ws + g.zda + 16L * K * l;
    const int eop = top ? E_TANH_D : E_GATE;
    const double* aux = top ? tz : zs + 16L * K * l;
    if (l == 0) tgemm(th + n.o.Win + n.d + 1, ld, 1, K, H, in, A_PLAIN, nullptr, nullptr, 0, 0.0, ws + x.vxp, eop, aux, out);
    else tgemm(th + n.o.Wh, K, 1, K, K, in, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, eop, aux, out);
    in = out;
  }
}

// tfield_vjp_tan with a stage time PER PATH and a slab: for (a, ad) at (t, yin) with the tangent yind of yin -- gy, gyd (overwritten),
// Sx += dz_0, Sxd += dzd_0, and into slab the TANGENT of vfield_vjp's updates: outer(dzd, in) + outer(dz, ind) per layer, the bias
// rows and Win's time column from dzd alone.  fo (may be null): F(t, yin).
__device__ void gfield_vjp_tan(const Net& n, const TileWork& w, const HvpWork& x, const GvjpWork& g, double* ws, double t,
                               const double* yin, const double* yind, const double* a, const double* ad, double* gy, double* gyd,
                               double* slab, double* fo) {
  const int K = n.K, H = n.H, ld = n.o.ldin;
  const double* th = n.th;
  double* tv = ws + g.tv;
  if (lane_id() < 16) tv[lane_id()] = t;                         // (ordered before its reader by tfield's sync_tile)
  tfield(n, w, ws, t, yin, fo, true);
  gfield_tan(n, w, x, g, ws, yind);
  const double* zs = ws + w.zs;
  const double* tz = ws + w.th;
  const double* thd = ws + x.thd;
  const double* zda = ws + g.zda;
  double* q = ws + x.q;
  double* dz = ws + w.dz;
  double* dzp = ws + w.dzp;
  double* dzd = ws + x.dzd;
  double* dzpd = ws + x.dzpd;
  double* Sx = ws + w.total - 16L * K;
  double* Sxd = ws + x.sxd;
  // dz = (Wo^T a) (1 - tanh^2); dzd = (Wo^T ad) (1 - tanh^2) - 2 (Wo^T a) tz thd
  tgemm(th + n.o.Wo, 1, K, K, H, a, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_TANH_D, tz, dz);
  tgemm(th + n.o.Wo, 1, K, K, H, a, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, q);
  tgemm(th + n.o.Wo, 1, K, K, H, ad, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_TANH_D, tz, dzd);
  for (int e = lane_id(); e < 16 * K; e += 64) dzd[e] -= 2.0 * q[e] * tz[e] * thd[e];
  sync_tile();
  touter(slab, n.o.Wo, K, H, K, ad, tz, A_PLAIN);
  touter(slab, n.o.Wo, K, H, K, a, thd, A_PLAIN);
  trowsum(slab, n.o.Wob, 1, H, ad, nullptr, 1.0);
  for (int l = n.m - 1; l >= 1; --l) {
    const double* zp = zs + 16L * K * (l - 1);
    touter(slab, n.o.Wh, K, K, K, dzd, zp, A_RELU);
    touter(slab, n.o.Wh, K, K, K, dz, zda + 16L * K * (l - 1), A_PLAIN);
    trowsum(slab, n.o.Whb, 1, K, dzd, nullptr, 1.0);
    tgemm(th + n.o.Wh, 1, K, K, K, dz, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, zp, dzp);
    tgemm(th + n.o.Wh, 1, K, K, K, dzd, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, zp, dzpd);
    double* s_ = dz; dz = dzp; dzp = s_;
    s_ = dzd; dzd = dzpd; dzpd = s_;
  }
  touter(slab, (long)n.o.Win + n.d + 1, ld, K, H, dzd, yin, A_PLAIN);
  touter(slab, (long)n.o.Win + n.d + 1, ld, K, H, dz, yind, A_PLAIN);
  trowsum(slab, (long)n.o.Win + n.d, ld, K, dzd, tv, 1.0);
  for (int e = lane_id(); e < 16 * K; e += 64) Sx[e] += dz[e], Sxd[e] += dzd[e];
  // gy = Win[:, d+1:]^T dz, gyd = Win[:, d+1:]^T dzd
  tgemm(th + n.o.Win + n.d + 1, 1, ld, H, K, dz, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, gy);
  tgemm(th + n.o.Win + n.d + 1, 1, ld, H, K, dzd, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, gyd);
}

// tstep_rk4_bwd_tan (xw_tiled_paths_hvp.hip) on gfield_vjp_tan: v.lam and vd.lam, the cotangent of y_l and its tangent, become those
// of y_{l-1} (v.Y1, vd.Y1)
__device__ void gstep_rk4_bwd_tan(const Net& n, const TileWork& w, const HvpWork& x, const GvjpWork& g, double* ws, double t0, double dt,
                                  const SweepVecs& v, const SweepVecs& vd, double* slab) {
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
  gfield_vjp_tan(n, w, x, g, ws, t0 + dt, v.Y4, vd.Y4, v.a, vd.a, v.g4, vd.g4, slab, nullptr);
  tcomb(H, v.a, nullptr, 3 * dt / 8, v.lam, dt, v.g4);
  tcomb(H, vd.a, nullptr, 3 * dt / 8, vd.lam, dt, vd.g4);
  gfield_vjp_tan(n, w, x, g, ws, t0 + 2 * dt / 3, v.Y3, vd.Y3, v.a, vd.a, v.g3, vd.g3, slab, nullptr);
  tcomb(H, v.a, nullptr, 3 * dt / 8, v.lam, -dt, v.g4, dt, v.g3);
  tcomb(H, vd.a, nullptr, 3 * dt / 8, vd.lam, -dt, vd.g4, dt, vd.g3);
  gfield_vjp_tan(n, w, x, g, ws, t0 + dt / 3, v.Y2, vd.Y2, v.a, vd.a, v.g2, vd.g2, slab, nullptr);
  for (int e = lane_id(); e < 16 * H; e += 64) {
    v.a[e] = (dt / 8) * v.lam[e] + dt * v.g4[e] - (dt / 3) * v.g3[e] + (dt / 3) * v.g2[e];
    vd.a[e] = (dt / 8) * vd.lam[e] + dt * vd.g4[e] - (dt / 3) * vd.g3[e] + (dt / 3) * vd.g2[e];
  }
  sync_tile();
  gfield_vjp_tan(n, w, x, g, ws, t0, v.Y1, vd.Y1, v.a, vd.a, v.gy, vd.gy, slab, nullptr);
  for (int e = lane_id(); e < 16 * H; e += 64) {
    v.lam[e] += v.g4[e] + v.g3[e] + v.g2[e] + v.gy[e];
    vd.lam[e] += vd.g4[e] + vd.g3[e] + vd.g2[e] + vd.gy[e];
  }
  sync_tile();
}

__global__ void __launch_bounds__(64) kt_paths_gvjp(XwPathsGvjpJob job, const double* __restrict__ theta, int method, int L, int d,
                                                     int H, int K, int m, double* __restrict__ work) {
  const int N = job.N, p0 = blockIdx.x * 16;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TileWork w = tile_work(1, d, H, K, m);
  const HvpWork x = hvp_work(w, d, H, K);
  const GvjpWork g = gvjp_work(x, K, m);
  double* ws = work + (long)blockIdx.x * g.total;
  double* slab = job.gslab + (long)blockIdx.x * n.o.total;
  const SweepVecs v = sweep_vecs(ws + w.hv, H), vd = sweep_vecs(ws + x.hvd, H);
  double* wuv = ws + w.ub;                                         // the weights on u, ...
  double* wtv = ws + g.wt;                                         //   ... on ut
  double* st = ws + w.st;
  double* vsv = ws + x.vs;
  double* Sx = ws + w.total - 16L * K;
  double* Sxd = ws + x.sxd;
  const int l16 = lane_id() & 15;
  const bool lane_active = p0 + l16 < N;
  const int pc = lane_active ? p0 + l16 : N - 1;                   // the lane's own path
  const double* flw = theta + n.o.FLw;
  const int ns = tile_steps(job.nstep, N, p0, L);
  // prologue: the start values; the weights and the direction, exactly 0 past the end of the job and where the job has none;
  // Sx = Sxd = 0; the tile's x, xproj and vxp = Win[:, 0..d) vx
  if (lane_id() < 16) {
    st[l16] = job.start[pc];
    wuv[l16] = (job.wu && lane_active) ? job.wu[p0 + l16] : 0.0;
    wtv[l16] = (job.wt && lane_active) ? job.wt[p0 + l16] : 0.0;
    vsv[l16] = (job.vs && lane_active) ? job.vs[p0 + l16] : 0.0;
  }
  for (int e = lane_id(); e < 16 * K; e += 64) Sx[e] = 0.0, Sxd[e] = 0.0;
  tload0(d, N, p0, job.vx, ws + x.vxt);
  tile_x(n, w, ws, job.xT, N, p0);                                   // (its sync_tile orders the loads above as well)
  tgemm(theta + n.o.Win, n.o.ldin, 1, K, d, ws + x.vxt, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, ws + x.vxp);
  // the top of the sweep, at row ns: lam = FL_w, lamd = wu FL_w + wt (dF/dy)^T FL_w; the read-out's and, under wt, the field's slab
  tload(H, N, p0, job.Y + (long)ns * H * N, v.Y1);
  tload0(H, N, p0, job.vx ? job.Yd + (long)ns * H * N : nullptr, vd.Y1);
  sync_tile();
  if (job.wt) {
    for (int e = lane_id(); e < 16 * H; e += 64) v.a[e] = 0.0, vd.a[e] = flw[e >> 4] * wtv[e & 15];
    sync_tile();
    gfield_vjp_tan(n, w, x, g, ws, job.tT[(long)ns * N + pc], v.Y1, vd.Y1, v.a, vd.a, v.gy, vd.gy, slab, v.fo);
    for (int e = lane_id(); e < 16 * H; e += 64) {
      v.lam[e] = flw[e >> 4];
      vd.lam[e] = fma(flw[e >> 4], wuv[e & 15], vd.gy[e]);
      vd.fo[e] = fma(wtv[e & 15], v.fo[e], fma(wuv[e & 15], v.Y1[e], vd.Y1[e]));
    }
  } else {
    for (int e = lane_id(); e < 16 * H; e += 64) {
      v.lam[e] = flw[e >> 4];
      vd.lam[e] = flw[e >> 4] * wuv[e & 15];
      vd.fo[e] = fma(wuv[e & 15], v.Y1[e], vd.Y1[e]);
    }
  }
  sync_tile();
  // FL_w += sum_p (wu y_ns + yd_ns + wt F), FL_b += sum_p wu
  trowsum(slab, n.o.FLw, 1, H, vd.fo, nullptr, 1.0);
  if (lane_id() == 0) {
    double s = 0.0;
    for (int p = 0; p < 16; ++p) s += wuv[p];
    slab[n.o.FLb] += s;
  }
  sync_tile();
  for (int l = ns; l >= 1; --l) {
    tload(H, N, p0, job.Y + (long)(l - 1) * H * N, v.Y1);
    tload0(H, N, p0, job.vx ? job.Yd + (long)(l - 1) * H * N : nullptr, vd.Y1);
    sync_tile();
    // y_l = step(y_{l-1}): (lam, lamd) become those of y_{l-1}; kt_paths_hvp's text on gfield_vjp_tan
    const double t0 = job.tT[(long)(l - 1) * N + pc], dt = job.tT[(long)l * N + pc] - t0;
    if (method == 0) {
      tcomb(H, v.a, nullptr, dt, v.lam);
      tcomb(H, vd.a, nullptr, dt, vd.lam);
      gfield_vjp_tan(n, w, x, g, ws, t0, v.Y1, vd.Y1, v.a, vd.a, v.gy, vd.gy, slab, nullptr);
      tcomb(H, v.lam, v.lam, 1.0, v.gy);
      tcomb(H, vd.lam, vd.lam, 1.0, vd.gy);
    } else if (method == 1) {
      tfield(n, w, ws, t0, v.Y1, v.fo, true);
      tfield_tan(n, w, x, ws, vd.Y1, vd.fo);
      tcomb(H, v.Y2, v.Y1, dt / 2, v.fo);
      tcomb(H, vd.Y2, vd.Y1, dt / 2, vd.fo);
      tcomb(H, v.a, nullptr, dt, v.lam);
      tcomb(H, vd.a, nullptr, dt, vd.lam);
      gfield_vjp_tan(n, w, x, g, ws, t0 + dt / 2, v.Y2, vd.Y2, v.a, vd.a, v.gy, vd.gy, slab, nullptr);
      tcomb(H, v.lam, v.lam, 1.0, v.gy);
      tcomb(H, vd.lam, vd.lam, 1.0, vd.gy);
      tcomb(H, v.a, nullptr, dt / 2, v.gy);
      tcomb(H, vd.a, nullptr, dt / 2, vd.gy);
      gfield_vjp_tan(n, w, x, g, ws, t0, v.Y1, vd.Y1, v.a, vd.a, v.gy, vd.gy, slab, nullptr);
      tcomb(H, v.lam, v.lam, 1.0, v.gy);
      tcomb(H, vd.lam, vd.lam, 1.0, vd.gy);
    } else {
      gstep_rk4_bwd_tan(n, w, x, g, ws, t0, dt, v, vd, slab);
    }
  }
  // tail: kt_paths_vjp's, every update with its tangent.  The lift 1 -> H -> H -> H reversed on lam and on lamd (piecewise linear:
  // its gates from the lift itself), its inputs' tangents along vs (kt_paths_jvp's prologue); the x columns and the bias of Win
  double *p0v = v.Y2, *p2v = v.Y3, *y0 = v.Y4, *dh2 = v.fo, *dh1 = v.g4, *p0d = vd.Y2, *p2d = vd.Y3, *dh2d = vd.fo, *dh1d = vd.g4;
  tlift(n, st, p0v, p2v, y0);
  for (int e = lane_id(); e < 16 * H; e += 64) p0d[e] = p0v[e] > 0.0 ? theta[n.o.IL0w + (e >> 4)] * vsv[e & 15] : 0.0;
  sync_tile();
  tgemm(theta + n.o.IL2w, H, 1, H, H, p0d, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p2v, p2d);
  tgemm(theta + n.o.IL4w, 1, H, H, H, v.lam, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p2v, dh2);
  tgemm(theta + n.o.IL2w, 1, H, H, H, dh2, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p0v, dh1);
  tgemm(theta + n.o.IL4w, 1, H, H, H, vd.lam, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p2v, dh2d);
  tgemm(theta + n.o.IL2w, 1, H, H, H, dh2d, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p0v, dh1d);
  touter(slab, n.o.IL4w, H, H, H, vd.lam, p2v, A_RELU);
  touter(slab, n.o.IL4w, H, H, H, v.lam, p2d, A_PLAIN);
  touter(slab, n.o.IL2w, H, H, H, dh2d, p0v, A_RELU);
  touter(slab, n.o.IL2w, H, H, H, dh2, p0d, A_PLAIN);
  trowsum(slab, n.o.IL4b, 1, H, vd.lam, nullptr, 1.0);
  trowsum(slab, n.o.IL2b, 1, H, dh2d, nullptr, 1.0);
  trowsum(slab, n.o.IL0w, 1, H, dh1d, st, 1.0);
  trowsum(slab, n.o.IL0w, 1, H, dh1, vsv, 1.0);
  trowsum(slab, n.o.IL0b, 1, H, dh1d, nullptr, 1.0);
  trowsum(slab, n.o.Winb, 1, K, Sxd, nullptr, 1.0);
  touter(slab, n.o.Win, n.o.ldin, K, d, Sxd, ws + w.xt, A_PLAIN);
  touter(slab, n.o.Win, n.o.ldin, K, d, Sx, ws + x.vxt, A_PLAIN);
}

}  // namespace

// ---- entry points (include/xnwan_grad_vjp.h) --------------------------------------------------------------------------------------
extern "C" int xw_paths_tiled_gvjp_work(int d, int H, int K, int m) {
  if (!xw_tiled_ode_ok(d, H, K, m)) return -1;
  return (int)gvjp_work(hvp_work(tile_work(1, d, H, K, m), d, H, K), K, m).total;
}

extern "C" int xw_paths_tiled_gvjp(const XwPathsGvjpJob* jobs, int njobs, const double* theta, int method, int L, int d, int H, int K,
                                   int m, double* work, void* stream) {
  if (!jobs || njobs < 1 || !theta || !work || L < 1 || method < 0 || method > 2) return XW_E_ARG;
  if (!xw_tiled_ode_ok(d, H, K, m)) return XW_E_DIMS;
  for (int i = 0; i < njobs; ++i) {
    const XwPathsGvjpJob& j = jobs[i];
    if (!j.xT || !j.start || !j.tT || !j.Y || !j.gslab || j.N < 1) return XW_E_ARG;
    if (!j.vx != !j.vs || (j.vx && !j.Yd) || !(j.wu || j.wt || j.vx)) return XW_E_ARG;
  }
  const long per = gvjp_work(hvp_work(tile_work(1, d, H, K, m), d, H, K), K, m).total, P = u_offsets(d, H, K).total;
  long off = 0;
  for (int i = 0; i < njobs; ++i) {
    const int tiles = (jobs[i].N + 15) / 16;
    const hipError_t e = hipMemsetAsync(jobs[i].gslab, 0, sizeof(double) * P * tiles, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kt_paths_gvjp, dim3(tiles), dim3(64), 0, (hipStream_t)stream, jobs[i], theta, method, L, d, H, K, m, work + off);
    off += per * tiles;
  }
  return xw_launch_status();
}
