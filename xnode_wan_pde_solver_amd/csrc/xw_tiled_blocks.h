// xw_tiled_blocks.h -- the building blocks of the tiled stepper family (xw_tiled.hip): the per-tile workspace and the tile
// products, field, VJP, lift and combinations that its kernels -- and the tiled dopri5 kernels of xw_tdopri.hip -- are written
// with.  Library-internal; included INSIDE an anonymous namespace, after xw_common.h and xnwan.h.
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

// ---- per-path siblings (xw_tiled_paths.hip): every path of the tile on a time grid of its own ---------------------------------
// The time t_p and the coefficients c*_p are PER LANE: the value of the lane's own path, column lane & 15.  tgemm's epilogue
// (e = r * 16 + (lane & 15)) and tcomb's loop (e = lane + 64 i) touch columns e & 15 == lane & 15 only, so the originals, handed a
// lane's own value, ARE the per-path forms: the same operations in the same order -- bias, fma(tcol[r], t_p, .), add;
// fma(c_p, s1[e], v) -- and, on a tile whose 16 paths carry one grid, the same bits as with the scalar.  (tfield hands its time
// to the time term of z_0's tgemm and nowhere else.)
__device__ __forceinline__ void tfield_pp(const Net& n, const TileWork& w, double* ws, double t_p, const double* yin, double* fo) {
  tfield(n, w, ws, t_p, yin, fo, false);
}
__device__ __forceinline__ void tcomb_pp(int H, double* dst, const double* s0, double c1_p, const double* s1, double c2_p = 0.0,
                                         const double* s2 = nullptr, double c3_p = 0.0, const double* s3 = nullptr) {
  tcomb(H, dst, s0, c1_p, s1, c2_p, s2, c3_p, s3);
}

__device__ __forceinline__ void set_prio(int drop) {
  switch (3 - (drop & 3)) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
  }
}
