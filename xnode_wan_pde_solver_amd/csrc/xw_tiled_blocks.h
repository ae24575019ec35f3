// xw_tiled_blocks.h -- the building blocks of the tiled stepper family: the per-tile workspace; the tile products, field, VJP, lift
// and combinations; and the sequences its kernels share -- the fixed-grid step, the rk4 reverse, the output block, the cotangent on
// u of a time index, the sweeps' prologue and tail.  Used by xw_tiled.hip, xw_tiled_paths.hip,
// xw_tdopri.hip and xw_tdopri_paths.hip; kt_ode_bwd alone keeps its own text of the sweep pieces (xw_tiled.hip says why).  Library-internal; included INSIDE an anonymous namespace, after xw_common.h, xnwan.h and
// xw_generic_cot.h (cot_u; the host's check of a sweep job, sweep_job_ok, is there too).
#pragma once

#define XWT_MAX_H 256
#define XWT_MAX_K 256
#define XWT_MAX_M 32

// ---- the per-tile workspace: every vector is [rows][16] doubles -------------------------------------------------------------
struct TileWork {
  long xt, xp, zs, th, dz, dzp, hv, ub, st, total;   // (offsets in doubles; hv: the first of nh H-vectors)
  int nh;
};
__host__ __device__ inline TileWork tile_work(int sweep, int d, int H, int K, int m) {
  TileWork w;
  long p = 0;
  const int nz = sweep ? m : 2;                      // forward: two K-vectors in turn; sweep: every layer's pre-activation
  w.xt = p; p += 32L * d;                            // x of the 16 paths (sweep: then d/dx of them)
  w.xp = p; p += 16L * K;                            // Win[:, 0..d) x + Win.b (hoisted: x does not move along a path)
  w.zs = p; p += 16L * K * nz;
  w.th = p; p += 16L * K;                            // tanh of the last pre-activation
  w.dz = p; p += 16L * K;                            // (sweep) cotangents of a layer's pre-activation, ...
  w.dzp = p; p += 16L * K;                           //   ... of the one below, and Sx: the summed cotangent of z_0
  w.nh = sweep ? 12 : 5;
  w.hv = p; p += 16L * H * w.nh;
  w.ub = p; p += 16;                                 // cotangent on u of the current time index
  w.st = p; p += 16;                                 // start values
  p += 16L * K;                                      // (sweep: Sx)
  w.total = p;
  return w;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x; }
__device__ __forceinline__ void sync_tile() { __syncthreads(); }   // one wave per workgroup: orders the phases' global traffic

enum { A_PLAIN = 0, A_RELU = 1 };
enum { E_NONE = 0, E_TANH_D = 1, E_GATE = 2 };

// out[r][p] = init(r, p) + sum_c W(r, c) A[c][p],  r < R, c < C;  W(r, c) = W[r wr + c wc] (so transposed products are the same
// loop), A gated by relu when aop == A_RELU; init = bias[r] (may be null) + tcol[r] * t (may be null) + add[r][p] (may be null);
// epilogue E_TANH_D: times (1 - g^2) with g = aux[r][p] (tanh values), E_GATE: zero where aux[r][p] <= 0.
// MFMA: A-operand W(r0 + (l & 15), c0 + (l >> 4)), B-operand A[c0 + (l >> 4)][l & 15]; D row r0 + (l >> 4) + 4 i, column l & 15.
__device__ void tgemm(const double* __restrict__ W, long wr, long wc, int R, int C, const double* A, int aop, const double* bias,
                      const double* tcol, long tcs, double t, const double* add, int eop, const double* aux, double* out) {
  const int l = lane_id(), lr = l & 15, lk = l >> 4;
  for (int r0 = 0; r0 < R; r0 += 16) {
    const int ra = r0 + lr;
    const bool rok = ra < R;
    const double* wrow = W + (long)(rok ? ra : 0) * wr;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < C; c0 += 4) {
      const int c = c0 + lk;
      const bool cok = c < C;
      const double wa = (rok && cok) ? wrow[(long)c * wc] : 0.0;
      double b = cok ? A[c * 16 + lr] : 0.0;
      if (aop == A_RELU) b = b > 0.0 ? b : 0.0;
      acc = XW_MFMA(wa, b, acc);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + lk + 4 * i;
      if (r >= R) continue;
      const int e = r * 16 + lr;
      double v = acc[i];
      if (bias) v += bias[r];
      if (tcol) v = fma(tcol[(long)r * tcs], t, v);
      if (add) v += add[e];
      if (eop == E_TANH_D) v *= 1.0 - aux[e] * aux[e];
      else if (eop == E_GATE) v = aux[e] > 0.0 ? v : 0.0;
      out[e] = v;
    }
  }
  sync_tile();
}

// slab[e0 + r ld + c] += sum_p U[r][p] V[c][p] (V gated by relu when vop == A_RELU), r < R, c < C: the 16 paths are the
// reduction dimension (four k-steps).  A-operand U[r0 + (l & 15)][k], B-operand V[c0 + (l & 15)][k], k = 4 s + (l >> 4);
// entry (r0 + (l >> 4) + 4 i, c0 + (l & 15)) belongs to one lane, always the same one.
__device__ void touter(double* slab, long e0, int ld, int R, int C, const double* U, const double* V, int vop) {
  const int l = lane_id(), lr = l & 15, lk = l >> 4;
  for (int r0 = 0; r0 < R; r0 += 16) {
    const int ra = r0 + lr;
    double ua[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) ua[s] = ra < R ? U[ra * 16 + 4 * s + lk] : 0.0;
    for (int c0 = 0; c0 < C; c0 += 16) {
      const int ca = c0 + lr;
      d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        double v = ca < C ? V[ca * 16 + 4 * s + lk] : 0.0;
        if (vop == A_RELU) v = v > 0.0 ? v : 0.0;
        acc = XW_MFMA(ua[s], v, acc);
      }
      const int c = c0 + lr;
      if (c < C) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = r0 + lk + 4 * i;
          if (r < R) slab[e0 + (long)r * ld + c] += acc[i];
        }
      }
    }
  }
}

// slab[e0 + r stride] += scale sum_p U[r][p] (w ? w[p] : 1), r < R -- bias gradients and the like; paths summed in order
__device__ void trowsum(double* slab, long e0, long stride, int R, const double* U, const double* w, double scale) {
  for (int r = lane_id(); r < R; r += 64) {
    double s = 0.0;
    for (int p = 0; p < 16; ++p) s = w ? fma(U[r * 16 + p], w[p], s) : s + U[r * 16 + p];
    slab[e0 + (long)r * stride] += scale * s;
  }
}

struct Net {
  const double* th;
  UOff o;
  int d, H, K, m;
};

// fo = F(t, yin) for the tile (src/model.py:130-141, 153-156); the pre-activations land in zs (the forward: two K-vectors in
// turn, zs_all == false; the sweep: layer l at zs + 16 K l) and tanh(z_{m-1}) in th
__device__ void tfield(const Net& n, const TileWork& w, double* ws, double t, const double* yin, double* fo, bool zs_all) {
  const int K = n.K, H = n.H, ld = n.o.ldin;
  const double* th = n.th;
  double* zs = ws + w.zs;
  // z_0 = Win[:, d+1:] y + Win[:, d] t + xproj
  tgemm(th + n.o.Win + n.d + 1, ld, 1, K, H, yin, A_PLAIN, nullptr, th + n.o.Win + n.d, ld, t, ws + w.xp, E_NONE, nullptr, zs);
  double* z = zs;
  for (int l = 1; l < n.m; ++l) {
    double* zn = zs_all ? zs + 16L * K * l : zs + 16L * K * (l & 1);
    tgemm(th + n.o.Wh, K, 1, K, K, z, A_RELU, th + n.o.Whb, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, zn);
    z = zn;
  }
  double* tz = ws + w.th;
  for (int e = lane_id(); e < 16 * K; e += 64) tz[e] = xw_tanh(z[e]);
  sync_tile();
  if (fo) tgemm(th + n.o.Wo, K, 1, H, K, tz, A_PLAIN, th + n.o.Wob, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, fo);
}

// a^T dF/d(y, theta) at (t, yin): gy (overwritten), Sx += cotangent of z_0, parameter gradients into slab (or none)
__device__ void tfield_vjp(const Net& n, const TileWork& w, double* ws, double t, const double* yin, const double* a, double* gy,
                           double* slab) {
  const int K = n.K, H = n.H, ld = n.o.ldin;
  const double* th = n.th;
  tfield(n, w, ws, t, yin, nullptr, true);
  const double* zs = ws + w.zs;
  const double* tz = ws + w.th;
  double* dz = ws + w.dz;
  double* dzp = ws + w.dzp;
  double* Sx = ws + w.total - 16L * K;
  // dz = (Wo^T a) (1 - tanh^2)
  tgemm(th + n.o.Wo, 1, K, K, H, a, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_TANH_D, tz, dz);
  if (slab) {
    touter(slab, n.o.Wo, K, H, K, a, tz, A_PLAIN);
    trowsum(slab, n.o.Wob, 1, H, a, nullptr, 1.0);
  }
  for (int l = n.m - 1; l >= 1; --l) {
    const double* zp = zs + 16L * K * (l - 1);
    if (slab) {
      touter(slab, n.o.Wh, K, K, K, dz, zp, A_RELU);
      trowsum(slab, n.o.Whb, 1, K, dz, nullptr, 1.0);
    }
    tgemm(th + n.o.Wh, 1, K, K, K, dz, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, zp, dzp);
    double* s_ = dz; dz = dzp; dzp = s_;
  }
  if (slab) {
    touter(slab, (long)n.o.Win + n.d + 1, ld, K, H, dz, yin, A_PLAIN);
    trowsum(slab, (long)n.o.Win + n.d, ld, K, dz, nullptr, t);
  }
  for (int e = lane_id(); e < 16 * K; e += 64) Sx[e] += dz[e];
  // gy = Win[:, d+1:]^T dz
  tgemm(th + n.o.Win + n.d + 1, 1, ld, H, K, dz, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, gy);
}

// the tile's x (clamped to the last path past the end) and xproj = Win[:, 0..d) x + Win.b
__device__ void tile_x(const Net& n, const TileWork& w, double* ws, const double* xT, int N, int p0) {
  double* xt = ws + w.xt;
  for (int e = lane_id(); e < 16 * n.d; e += 64) {
    const int p = p0 + (e & 15);
    xt[e] = xT[(long)(e >> 4) * N + (p < N ? p : N - 1)];
  }
  sync_tile();
  tgemm(n.th + n.o.Win, n.o.ldin, 1, n.K, n.d, xt, A_PLAIN, n.th + n.o.Winb, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, ws + w.xp);
}

// y0 = IL(start) (src/model.py:78,97): pre0 = IL0 s, pre2 = IL2 relu(pre0), y = IL4 relu(pre2)
__device__ void tlift(const Net& n, const double* st, double* pre0, double* pre2, double* y) {
  const int H = n.H;
  const double* th = n.th;
  for (int e = lane_id(); e < 16 * H; e += 64) pre0[e] = fma(th[n.o.IL0w + (e >> 4)], st[e & 15], th[n.o.IL0b + (e >> 4)]);
  sync_tile();
  tgemm(th + n.o.IL2w, H, 1, H, H, pre0, A_RELU, th + n.o.IL2b, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, pre2);
  tgemm(th + n.o.IL4w, H, 1, H, H, pre2, A_RELU, th + n.o.IL4b, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, y);
}

// dst = src0 + c1 src1 (+ c2 src2 (+ c3 src3)) elementwise over an H-vector (null sources are skipped)
__device__ void tcomb(int H, double* dst, const double* s0, double c1, const double* s1, double c2 = 0.0, const double* s2 = nullptr,
                      double c3 = 0.0, const double* s3 = nullptr) {
  for (int e = lane_id(); e < 16 * H; e += 64) {
    double v = s0 ? s0[e] : 0.0;
    v = fma(c1, s1[e], v);
    if (s2) v = fma(c2, s2[e], v);
    if (s3) v = fma(c3, s3[e], v);
    dst[e] = v;
  }
  sync_tile();
}

// ---- tile <-> [rows][N] arrays -------------------------------------------------------------------------------------------------
// v[h][c] = src[h][p0 + c] of an [H][N] array, clamped to the last path (the caller orders it with sync_tile)
__device__ __forceinline__ void tload(int H, int N, int p0, const double* __restrict__ src, double* v) {
  for (int e = lane_id(); e < 16 * H; e += 64) {
    const int p = p0 + (e & 15);
    v[e] = src[(long)(e >> 4) * N + (p < N ? p : N - 1)];
  }
}
// the reverse, for the paths the job has
__device__ __forceinline__ void tstore(int H, int N, int p0, const double* v, double* __restrict__ dst) {
  for (int e = lane_id(); e < 16 * H; e += 64)
    if (p0 + (e & 15) < N) dst[(long)(e >> 4) * N + p0 + (e & 15)] = v[e];
}

// u[row] = FL(y) and (Y not null) Y[row] = y for the tile (y complete: behind a sync_tile)
__device__ __forceinline__ void tput_output(const Net& n, double* u, double* Y, long row, int N, int p0, const double* y) {
  const int l16 = lane_id() & 15, H = n.H;
  if (lane_id() < 16 && p0 + l16 < N) {
    const double* flw = n.th + n.o.FLw;
    double v = n.th[n.o.FLb];
    for (int h = 0; h < H; ++h) v = fma(flw[h], y[h * 16 + l16], v);
    u[row * N + p0 + l16] = v;
  }
  if (Y) tstore(H, N, p0, y, Y + row * H * N);
}

// ---- one step of the fixed-grid schemes (method 0 euler, 1 midpoint, 2 rk4 by the 3/8 rule) and its reverse ------------------
// t0 and dt are passed BY VALUE: one grid for the tile (kt_ode_fwd: wave-uniform) or PER LANE -- the value of the lane's own path,
// column lane & 15 (kt_ode_fwd_pp).  tgemm's epilogue (e = r * 16 + (lane & 15)) and tcomb's loop (e = lane + 64 i) touch columns
// e & 15 == lane & 15 only, so the blocks, handed a lane's own value, ARE the per-path forms: the same operations in the same order
// -- bias, fma(tcol[r], t_p, .), add; fma(c_p, s1[e], v) -- and, on a tile whose 16 paths carry one grid, the same bits as with the
// scalar.  (tfield hands its time to the time term of z_0's tgemm and nowhere else.)

// the rk4 step from an evaluated k1 = F(t0, y) (k1 may be fo): acc = k1 + 3 k2 + 3 k3 + k4, cc = k1 - k2
__device__ __forceinline__ void tstep_rk4(const Net& n, const TileWork& w, double* ws, double t0, double dt, double* y, const double* k1,
                                          double* acc, double* cc, double* tmp, double* fo) {
  const int H = n.H;
  tcomb(H, acc, nullptr, 1.0, k1);
  tcomb(H, cc, nullptr, 1.0, k1);
  tcomb(H, tmp, y, dt / 3, k1);
  tfield(n, w, ws, t0 + dt / 3, tmp, fo, false);
  tcomb(H, acc, acc, 3.0, fo);
  tcomb(H, tmp, y, dt, fo, -dt / 3, cc);
  tcomb(H, cc, cc, -1.0, fo);
  tfield(n, w, ws, t0 + 2 * dt / 3, tmp, fo, false);
  tcomb(H, acc, acc, 3.0, fo);
  tcomb(H, tmp, y, dt, cc, dt, fo);
  tfield(n, w, ws, t0 + dt, tmp, fo, false);
  tcomb(H, acc, acc, 1.0, fo);
  tcomb(H, y, y, dt / 8, acc);
}

// y <- the step from (t0, y) over dt; acc, cc, tmp, fo: scratch H-vectors
__device__ __forceinline__ void tstep_fwd(const Net& n, const TileWork& w, double* ws, int method, double t0, double dt, double* y,
                                          double* acc, double* cc, double* tmp, double* fo) {
  const int H = n.H;
  if (method == 0) {
    tfield(n, w, ws, t0, y, fo, false);
    tcomb(H, y, y, dt, fo);
  } else if (method == 1) {
    tfield(n, w, ws, t0, y, fo, false);
    tcomb(H, tmp, y, dt / 2, fo);
    tfield(n, w, ws, t0 + dt / 2, tmp, fo, false);
    tcomb(H, y, y, dt, fo);
  } else {
    tfield(n, w, ws, t0, y, fo, false);
    tstep_rk4(n, w, ws, t0, dt, y, fo, acc, cc, tmp, fo);
  }
}

// the H-vectors of a fixed-grid sweep (tile_work: nh = 12), by name
struct SweepVecs {
  double *lam, *Y1, *Y2, *Y3, *Y4, *cc, *fo, *g4, *g3, *g2, *a, *gy;
};
__device__ __forceinline__ SweepVecs sweep_vecs(double* hv, int H) {
  const long s = 16L * H;
  return {hv, hv + s, hv + 2 * s, hv + 3 * s, hv + 4 * s, hv + 5 * s, hv + 6 * s, hv + 7 * s, hv + 8 * s, hv + 9 * s, hv + 10 * s,
          hv + 11 * s};
}

// the reverse of the rk4 step y_l = step(y_{l-1}), y_{l-1} in v.Y1: v.lam, the cotangent of y_l, becomes that of y_{l-1}; the stages
// are recomputed, parameter gradients go to slab (or none).  k1b (may be null): a further cotangent on k1 = F(t0, y_{l-1}).
// For kt_adams_bwd's start-up steps; kt_ode_bwd keeps its own text of this sequence (see there).
__device__ __forceinline__ void tstep_rk4_bwd(const Net& n, const TileWork& w, double* ws, double t0, double dt, const SweepVecs& v,
                                              double* slab, const double* k1b) {
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
  tfield_vjp(n, w, ws, t0 + dt, Y4, a, g4, slab);
  tcomb(H, a, nullptr, 3 * dt / 8, lam, dt, g4);
  tfield_vjp(n, w, ws, t0 + 2 * dt / 3, Y3, a, g3, slab);
  tcomb(H, a, nullptr, 3 * dt / 8, lam, -dt, g4, dt, g3);
  tfield_vjp(n, w, ws, t0 + dt / 3, Y2, a, g2, slab);
  for (int e = lane_id(); e < 16 * H; e += 64) {
    double s = (dt / 8) * lam[e] + dt * g4[e] - (dt / 3) * g3[e] + (dt / 3) * g2[e];
    if (k1b) s = s + k1b[e];
    a[e] = s;
  }
  sync_tile();
  tfield_vjp(n, w, ws, t0, Y1, a, gy, slab);
  for (int e = lane_id(); e < 16 * H; e += 64) lam[e] += g4[e] + g3[e] + g2[e] + gy[e];
  sync_tile();
}

// ---- the sweeps' shared ends ----------------------------------------------------------------------------------------------------
// prologue: the start values, Sx = 0 and lam = 0, the tile's x and xproj
__device__ __forceinline__ void sweep_prologue(const Net& n, const TileWork& w, double* ws, const XwOdeBwdJob& job, int p0, double* lam) {
  const int N = job.N, l16 = lane_id() & 15;
  double* st = ws + w.st;
  double* Sx = ws + w.total - 16L * n.K;
  if (lane_id() < 16) st[l16] = job.start[p0 + l16 < N ? p0 + l16 : N - 1];
  for (int e = lane_id(); e < 16 * n.K; e += 64) Sx[e] = 0.0;
  for (int e = lane_id(); e < 16 * n.H; e += 64) lam[e] = 0.0;
  tile_x(n, w, ws, job.xT, N, p0);
}

// ub = the job's cotangent on u at time index l for the tile's paths, zero past the end of the job (the caller orders it)
__device__ __forceinline__ void tcot_ub(const XwOdeBwdJob& job, int l, int L, int p0, double* ub) {
  const int l16 = lane_id() & 15;
  if (lane_id() < 16) ub[l16] = p0 + l16 < job.N ? cot_u(job, l, L, p0 + l16) : 0.0;
}

// slab's read-out entries for the output state v under the cotangent ub (both complete: behind a sync_tile)
__device__ __forceinline__ void readout_grad(double* slab, const Net& n, const double* v, const double* ub) {
  trowsum(slab, n.o.FLw, 1, n.H, v, ub, 1.0);
  if (lane_id() == 0) {
    double s = 0.0;
    for (int p = 0; p < 16; ++p) s += ub[p];
    slab[n.o.FLb] += s;
  }
}

// the cotangent on u of time index l >= 1, whose output state is v (stored by the caller, needed with a slab only):
// lam += FL_w ub, the read-out's gradient into slab
__device__ __forceinline__ void tcot_output(const XwOdeBwdJob& job, const Net& n, int l, int L, int p0, double* ub, const double* v,
                                            double* lam, double* slab) {
  const double* flw = n.th + n.o.FLw;
  tcot_ub(job, l, L, p0, ub);
  sync_tile();
  for (int e = lane_id(); e < 16 * n.H; e += 64) lam[e] = fma(flw[e >> 4], ub[e & 15], lam[e]);
  if (slab) readout_grad(slab, n, v, ub);
  sync_tile();
}

// tail, l = 0: read-out, then the lift 1 -> H -> H -> H, the x columns and the bias of the input layer; lam: the cotangent of y_0
// from the steps.  With mode bit 2 the x-side outputs are those of the ALL-ONES cotangent while the parameter gradients use the
// job's own (xw_generic.hip kg_ode_bwd).  p0v .. dh1: six scratch H-vectors.
__device__ __forceinline__ void sweep_tail(const Net& n, const TileWork& w, double* ws, const XwOdeBwdJob& job, int L, int p0, int mode,
                                           double* slab, const double* lam, double* p0v, double* p2v, double* y0, double* l0,
                                           double* dh2, double* dh1) {
  const int N = job.N, d = n.d, H = n.H, K = n.K, l16 = lane_id() & 15;
  const bool want_x = (mode & 1) != 0, ones_x = (mode & 4) != 0;
  const double* theta = n.th;
  const double* flw = theta + n.o.FLw;
  double* ub = ws + w.ub;
  const double* st = ws + w.st;
  const double* Sx = ws + w.total - 16L * K;
  tcot_ub(job, 0, L, p0, ub);
  sync_tile();
  tlift(n, st, p0v, p2v, y0);
  if (slab) readout_grad(slab, n, y0, ub);
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 0 && !slab) continue;
    if (pass == 1 && !(want_x && job.gs != nullptr)) continue;
    const bool ones = pass == 1 && ones_x;
    for (int e = lane_id(); e < 16 * H; e += 64) l0[e] = fma(flw[e >> 4], ones ? 1.0 : ub[e & 15], lam[e]);
    sync_tile();
    tgemm(theta + n.o.IL4w, 1, H, H, H, l0, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p2v, dh2);
    tgemm(theta + n.o.IL2w, 1, H, H, H, dh2, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p0v, dh1);
    if (pass == 0) {
      touter(slab, n.o.IL4w, H, H, H, l0, p2v, A_RELU);
      touter(slab, n.o.IL2w, H, H, H, dh2, p0v, A_RELU);
      trowsum(slab, n.o.IL4b, 1, H, l0, nullptr, 1.0);
      trowsum(slab, n.o.IL2b, 1, H, dh2, nullptr, 1.0);
      trowsum(slab, n.o.IL0w, 1, H, dh1, st, 1.0);
      trowsum(slab, n.o.IL0b, 1, H, dh1, nullptr, 1.0);
      sync_tile();
    } else if (lane_id() < 16 && p0 + l16 < N) {
      double s = 0.0;
      for (int i = 0; i < H; ++i) s = fma(theta[n.o.IL0w + i], dh1[i * 16 + l16], s);
      job.gs[p0 + l16] = s;
    }
  }
  // the x columns and the bias of the input layer, from the summed cotangent of its pre-activation
  if (slab) {
    trowsum(slab, n.o.Winb, 1, K, Sx, nullptr, 1.0);
    touter(slab, n.o.Win, n.o.ldin, K, d, Sx, ws + w.xt, A_PLAIN);
  }
  if (want_x && job.gx != nullptr) {
    double* gxt = ws + w.xt + 16L * d;
    tgemm(theta + n.o.Win, 1, n.o.ldin, d, K, Sx, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, gxt);
    tstore(d, N, p0, gxt, job.gx);
  }
}

__device__ __forceinline__ void set_prio(int drop) {
  switch (3 - (drop & 3)) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
  }
}
