// xw_tiled_paths_jet.hip -- quadratic forms of the Hessian of u over a RAGGED group: a second-order FORWARD jet of every path's
// final value U_p(x, s) = FL(y_{n_p}) along R curves per path, gamma(eps) = (x + eps vx, s + eps vs + eps^2 / 2 qs)
// (include/xnwan_jet.h): ju = d/deps U(gamma), quu = d^2/deps^2 U(gamma) at 0.  Forward over forward: no reverse sweep, no
// checkpoints -- what a trace sum_k w_k v_k^T Hess(u) v_k needs, where xw_tiled_paths_hvp.hip builds whole Hessian rows.
//
// The lift and the hidden layers of the field are ReLU -- piecewise linear, their gates constants of the differentiation, as
// autograd takes them -- so y'' runs through the same gated linear chain as y' (without the direction's share vxp of z'_0: x is
// linear in eps), and the one curvature of the model is the tanh in front of the field's output layer:
//   (tanh z)'' = (1 - tz^2) z'' - 2 tz (1 - tz^2) z'^2     (tfield_jet; z' raw: the tanh factor is applied behind its use)
// One kernel, kt_paths_jet2, one wave per block, grid (tiles, R): the block of (tile, r) recomputes the primal trajectory of its 16
// paths from `start` with the forward's step text (tstep_fwd / tstep_rk4 of xw_tiled_blocks.h, line by line, on tfield and on
// tcomb's arithmetic: u has the bits of kt_ode_fwd_pp) and carries (y', y'') of direction r behind every stage; t0 and dt in a
// register per lane.  The two orders share their products (tgemm2: every weight loaded once) and their combinations (jcomb).  The blocks of direction 0 store u.  A zero-length step is the exact identity of all three orders (fma(0, k, y) == y), so a
// path's bits depend neither on its tile neighbours nor on the nstep hint nor on the other directions.  Time is not perturbed.
// Lanes past the end of a job walk with the last path and store nothing.  No LDS, no float atomics, no waits between blocks, no
// read-back: the launch can be captured.
// The workspace is this source's own (jet_work), per BLOCK: the tiled sweep's (tile_work(1, ...), which keeps every layer's
// pre-activation -- the gates -- and which the blocks of xw_tiled_blocks.h address; its reverse-only vectors dz, dzp and Sx serve
// the first-order chain here) with the second order's vectors behind it.
#include "xw_common.h"
#include "xnwan_jet.h"

namespace {
#include "xw_generic_cot.h"   // (not used here: the sweep helpers of xw_tiled_blocks.h name cot_u / cot_job_ok)
#include "xw_tiled_blocks.h"

// ---- the workspace: the sweep's, then the jet's own (offsets in doubles from the block's base) ------------------------------------
struct JetWork {
  long vxt, zdd, zr, zzr, hvx, vs, qs, total;
};
__host__ __device__ inline JetWork jet_work(const TileWork& w, int d, int H, int K) {
  JetWork x;
  long p = w.total;
  x.vxt = p; p += 16L * d;                            // vx of the 16 paths
  x.zdd = p; p += 32L * K;                            // second-order pre-activations, gated, two in turn (the first order's: dz, dzp)
  x.zr = p; p += 16L * K;                             // z'_{m-1} raw, then (tanh z_{m-1})'
  x.zzr = p; p += 16L * K;                            // z''_{m-1} raw, then (tanh z_{m-1})''
  x.hvx = p; p += 16L * H * 3;                        // H-vectors 12 .. 14 (0 .. 11: the sweep's twelve)
  x.vs = p; p += 16;                                  // vs and ...
  x.qs = p; p += 16;                                  // ... qs of the 16 paths
  x.total = p;
  return x;
}

// an H-vector of every order: the primal, the first and the second derivative along the curve
struct Jet {
  double *p, *d, *dd;
};

// tgemm (xw_tiled_blocks.h) on two right-hand sides at once, out1 = W A1 (+ add1), out2 = W A2, both through the epilogue eop
// (E_NONE or E_GATE on aux): every element of W is loaded once for the two orders, and the two accumulator chains are independent,
// so each sees tgemm's operations in tgemm's order -- the bits of two tgemm calls -- while the matrix pipe has two chains to interleave
__device__ void tgemm2(const double* __restrict__ W, long wr, long wc, int R, int C, const double* A1, const double* A2, const double* add1,
                       int eop, const double* aux, double* out1, double* out2) {
  const int l = lane_id(), lr = l & 15, lk = l >> 4;
  for (int r0 = 0; r0 < R; r0 += 16) {
    const int ra = r0 + lr;
    const bool rok = ra < R;
    const double* wrow = W + (long)(rok ? ra : 0) * wr;
    d4 acc1 = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < C; c0 += 4) {
      const int c = c0 + lk;
      const bool cok = c < C;
      const double wa = (rok && cok) ? wrow[(long)c * wc] : 0.0;
      const double b1 = cok ? A1[c * 16 + lr] : 0.0, b2 = cok ? A2[c * 16 + lr] : 0.0;
      acc1 = XW_MFMA(wa, b1, acc1);
      acc2 = XW_MFMA(wa, b2, acc2);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + lk + 4 * i;
      if (r >= R) continue;
      const int e = r * 16 + lr;
      double v1 = acc1[i], v2 = acc2[i];
      if (add1) v1 += add1[e];
      if (eop == E_GATE) {
        const bool on = aux[e] > 0.0;
        v1 = on ? v1 : 0.0;
        v2 = on ? v2 : 0.0;
      }
      out1[e] = v1;
      out2[e] = v2;
    }
  }
  sync_tile();
}

// (fo.d, fo.dd) = the first and second derivative of F(t, y(eps)) along the curve, behind tfield(.., zs_all = true) at (t, yin.p),
// whose z_l and tanh(z_{m-1}) it reads: z'_0 = Win[:, d+1:] y' + vxp, z''_0 = Win[:, d+1:] y'', z'_l = Wh gate(z'_{l-1}) and the
// same for z''; the top layer is left RAW, then th' = (1 - tz^2) z', th'' = (1 - tz^2) (z'' - 2 tz z'^2); f' = Wo th', f'' = Wo th''
__device__ void tfield_jet(const Net& n, const TileWork& w, const JetWork& x, double* ws, const Jet& yin, const Jet& fo) {
  const int K = n.K, H = n.H, ld = n.o.ldin;
  const double* th = n.th;
  const double* zs = ws + w.zs;
  const double* tz = ws + w.th;
  const double* vxp = ws + w.total - 16L * K;
  double* zr = ws + x.zr;
  double* zzr = ws + x.zzr;
  const double *in1 = yin.d, *in2 = yin.dd;
  for (int l = 0; l < n.m; ++l) {
    const bool top = l == n.m - 1;
    double* out1 = top ? zr : ws + ((l & 1) ? w.dzp : w.dz);
    double* out2 = top ? zzr : ws + x.zdd + 16L * K * (l & 1);
    const int eop = top ? E_NONE : E_GATE;
    const double* aux = top ? nullptr : zs + 16L * K * l;
    if (l == 0) tgemm2(th + n.o.Win + n.d + 1, ld, 1, K, H, in1, in2, vxp, eop, aux, out1, out2);
    else tgemm2(th + n.o.Wh, K, 1, K, K, in1, in2, nullptr, eop, aux, out1, out2);
    in1 = out1;
    in2 = out2;
  }
  for (int e = lane_id(); e < 16 * K; e += 64) {
    const double t = tz[e], s = 1.0 - t * t, z1 = zr[e], z2 = zzr[e];
    zr[e] = s * z1;
    zzr[e] = s * (z2 - 2.0 * t * z1 * z1);
  }
  sync_tile();
  tgemm2(th + n.o.Wo, K, 1, H, K, zr, zzr, nullptr, E_NONE, nullptr, fo.d, fo.dd);
}

// fo = F(t, yin) to second order
__device__ void jfield(const Net& n, const TileWork& w, const JetWork& x, double* ws, double t, const Jet& yin, const Jet& fo) {
  tfield(n, w, ws, t, yin.p, fo.p, true);
  tfield_jet(n, w, x, ws, yin, fo);
}

// tcomb on every order (the combinations are linear: the same coefficients), tcomb's operations in tcomb's order per element, one
// pass and one sync_tile for the three: dst = s0 + c1 s1 (+ c2 s2); dst may be s0 or s1 (elementwise)
__device__ void jcomb(int H, const Jet& dst, const Jet* s0, double c1, const Jet& s1, double c2 = 0.0, const Jet* s2 = nullptr) {
  for (int e = lane_id(); e < 16 * H; e += 64) {
    double vp = s0 ? s0->p[e] : 0.0, vd = s0 ? s0->d[e] : 0.0, vdd = s0 ? s0->dd[e] : 0.0;
    vp = fma(c1, s1.p[e], vp);
    vd = fma(c1, s1.d[e], vd);
    vdd = fma(c1, s1.dd[e], vdd);
    if (s2) {
      vp = fma(c2, s2->p[e], vp);
      vd = fma(c2, s2->d[e], vd);
      vdd = fma(c2, s2->dd[e], vdd);
    }
    dst.p[e] = vp;
    dst.d[e] = vd;
    dst.dd[e] = vdd;
  }
  sync_tile();
}

__global__ void __launch_bounds__(64) kt_paths_jet2(XwPathsJetJob job, const double* __restrict__ theta, int method, int L, int d, int H,
                                                     int K, int m, double* __restrict__ work) {
  const int N = job.N, p0 = blockIdx.x * 16, r = blockIdx.y;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TileWork w = tile_work(1, d, H, K, m);
  const JetWork x = jet_work(w, d, H, K);
  double* ws = work + ((long)blockIdx.x + (long)gridDim.x * r) * x.total;
  const long hs = 16L * H;
  double* hv = ws + w.hv;
  double* hvx = ws + x.hvx;
  // the forward's five H-vectors, by order: 0 .. 4 the primal's, 5 .. 9 the first order's, 10 .. 14 the second's
  const Jet y = {hv, hv + 5 * hs, hv + 10 * hs}, acc = {hv + hs, hv + 6 * hs, hv + 11 * hs}, cc = {hv + 2 * hs, hv + 7 * hs, hvx},
            tmp = {hv + 3 * hs, hv + 8 * hs, hvx + hs}, fo = {hv + 4 * hs, hv + 9 * hs, hvx + 2 * hs};
  const int l16 = lane_id() & 15;
  const int pc = p0 + l16 < N ? p0 + l16 : N - 1;                 // the lane's own path
  int ns = L - 1;                                                  // the tile's step count (the forward's rule)
  if (job.nstep) {
    int mx = 0;
    for (int q = 0; q < 16 && p0 + q < N; ++q) mx = job.nstep[p0 + q] > mx ? job.nstep[p0 + q] : mx;
    ns = mx < ns ? mx : ns;
  }
  // prologue: start values and the direction, x, xproj and vxp = Win[:, 0..d) vx (no bias)
  if (lane_id() < 16) {
    ws[w.st + l16] = job.start[pc];
    ws[x.vs + l16] = job.vs[(long)r * N + pc];
    ws[x.qs + l16] = job.qs ? job.qs[(long)r * N + pc] : 0.0;
  }
  tload(d, N, p0, job.vx + (long)r * d * N, ws + x.vxt);
  tile_x(n, w, ws, job.xT, N, p0);                                 // (its sync_tile orders the loads above as well)
  tgemm(theta + n.o.Win, n.o.ldin, 1, K, d, ws + x.vxt, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr,
        ws + w.total - 16L * K);
  // y_0 = IL(start); y'_0 = IL4 gate(IL2 gate(IL0_w vs)) and y''_0 the same on qs: the lift is piecewise linear, its gates its own
  tlift(n, ws + w.st, acc.p, cc.p, y.p);
  for (int e = lane_id(); e < 16 * H; e += 64) {
    const bool on = acc.p[e] > 0.0;
    const double w0 = theta[n.o.IL0w + (e >> 4)];
    acc.d[e] = on ? w0 * ws[x.vs + (e & 15)] : 0.0;
    acc.dd[e] = on ? w0 * ws[x.qs + (e & 15)] : 0.0;
  }
  sync_tile();
  tgemm2(theta + n.o.IL2w, H, 1, H, H, acc.d, acc.dd, nullptr, E_GATE, cc.p, cc.d, cc.dd);
  tgemm2(theta + n.o.IL4w, H, 1, H, H, cc.d, cc.dd, nullptr, E_NONE, nullptr, y.d, y.dd);
  for (int l = 1; l <= ns; ++l) {
    const double t0 = job.tT[(long)(l - 1) * N + pc], dt = job.tT[(long)l * N + pc] - t0;
    // tstep_fwd's text on all three orders
    if (method == 0) {
      jfield(n, w, x, ws, t0, y, fo);
      jcomb(H, y, &y, dt, fo);
    } else if (method == 1) {
      jfield(n, w, x, ws, t0, y, fo);
      jcomb(H, tmp, &y, dt / 2, fo);
      jfield(n, w, x, ws, t0 + dt / 2, tmp, fo);
      jcomb(H, y, &y, dt, fo);
    } else {                                                       // (tstep_rk4: acc = k1 + 3 k2 + 3 k3 + k4, cc = k1 - k2)
      jfield(n, w, x, ws, t0, y, fo);
      jcomb(H, acc, nullptr, 1.0, fo);
      jcomb(H, cc, nullptr, 1.0, fo);
      jcomb(H, tmp, &y, dt / 3, fo);
      jfield(n, w, x, ws, t0 + dt / 3, tmp, fo);
      jcomb(H, acc, &acc, 3.0, fo);
      jcomb(H, tmp, &y, dt, fo, -dt / 3, &cc);
      jcomb(H, cc, &cc, -1.0, fo);
      jfield(n, w, x, ws, t0 + 2 * dt / 3, tmp, fo);
      jcomb(H, acc, &acc, 3.0, fo);
      jcomb(H, tmp, &y, dt, cc, dt, &fo);
      jfield(n, w, x, ws, t0 + dt, tmp, fo);
      jcomb(H, acc, &acc, 1.0, fo);
      jcomb(H, y, &y, dt / 8, acc);
    }
  }
  if (r == 0 && job.u) tput_output(n, job.u, nullptr, 0, N, p0, y.p);
  if (lane_id() < 16 && p0 + l16 < N) {
    const double* flw = theta + n.o.FLw;
    double s1 = 0.0, s2 = 0.0;
    for (int h = 0; h < H; ++h) {
      s1 = fma(flw[h], y.d[h * 16 + l16], s1);
      s2 = fma(flw[h], y.dd[h * 16 + l16], s2);
    }
    if (job.ju) job.ju[(long)r * N + p0 + l16] = s1;
    if (job.quu) job.quu[(long)r * N + p0 + l16] = s2;
  }
}

}  // namespace

// ---- entry points (include/xnwan_jet.h) -------------------------------------------------------------------------------------------
extern "C" int xw_paths_tiled_jet_work(int d, int H, int K, int m) {
  if (!xw_tiled_ode_ok(d, H, K, m)) return -1;
  return (int)jet_work(tile_work(1, d, H, K, m), d, H, K).total;
}

extern "C" int xw_paths_tiled_jet(const XwPathsJetJob* jobs, int njobs, const double* theta, int method, int L, int d, int H, int K,
                                  int m, double* work, void* stream) {
  if (!jobs || njobs < 1 || !theta || !work || L < 1 || method < 0 || method > 2) return XW_E_ARG;
  if (!xw_tiled_ode_ok(d, H, K, m)) return XW_E_DIMS;
  for (int i = 0; i < njobs; ++i) {
    const XwPathsJetJob& j = jobs[i];
    if (!j.xT || !j.start || !j.tT || !j.vx || !j.vs || !(j.ju || j.quu) || j.N < 1 || j.R < 1 || j.R > 65535) return XW_E_ARG;
  }
  const long per = jet_work(tile_work(1, d, H, K, m), d, H, K).total;
  long off = 0;
  for (int i = 0; i < njobs; ++i) {
    const int tiles = (jobs[i].N + 15) / 16;
    hipLaunchKernelGGL(kt_paths_jet2, dim3(tiles, jobs[i].R), dim3(64), 0, (hipStream_t)stream, jobs[i], theta, method, L, d, H, K, m,
                       work + off);
    off += per * tiles * jobs[i].R;
  }
  return xw_launch_status();
}
