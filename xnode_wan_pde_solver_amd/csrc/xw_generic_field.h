// xw_generic_field.h -- u_theta per path on the vector ALU: the field, its vector-Jacobian product, the lift and the
// x-projection, the deterministic slab accumulation and the read-out's gradient (xw_generic.hip; also the dopri5 kernels of
// xw_dopri.hip).
// Library-internal; included INSIDE an anonymous namespace, after xw_common.h and xw_generic.h.
#pragma once
constexpr int GH = XWG_MAX_H, GK = XWG_MAX_K, GW = XWG_MAX_W, GM = XWG_MAX_M, GQ = XWG_MAX_Q;

__device__ __forceinline__ double gsum16(double x) {       // sum over the 16 lanes (paths) that share a slab
  x += __shfl_xor(x, 1);
  x += __shfl_xor(x, 2);
  x += __shfl_xor(x, 4);
  x += __shfl_xor(x, 8);
  return x;
}
__device__ __forceinline__ double gsum64(double x) {       // sum over the wave
  x = gsum16(x);
  x += __shfl_xor(x, 16);
  x += __shfl_xor(x, 32);
  return x;
}

// ---- u_theta -------------------------------------------------------------------------------------------------------------------
struct Net {
  const double* th;
  UOff o;
  int d, H, K, m;
};

// out[r] = init[r] + sum_c Wm[r ldw + c] x(c), r < rows -- four rows at a time (four independent chains, every x(c) used four times)
template <class FX>
__device__ __forceinline__ void matvec(const double* Wm, int ldw, int rows, int cols, FX x, const double* init, double* out) {
  for (int r = 0; r < rows; r += 4) {
    const int r1 = r + 1 < rows ? r + 1 : rows - 1, r2 = r + 2 < rows ? r + 2 : rows - 1, r3 = r + 3 < rows ? r + 3 : rows - 1;
    const double* w0 = Wm + (long)r * ldw;
    const double* w1 = Wm + (long)r1 * ldw;
    const double* w2 = Wm + (long)r2 * ldw;
    const double* w3 = Wm + (long)r3 * ldw;
    double a0 = init ? init[r] : 0.0, a1 = init ? init[r1] : 0.0, a2 = init ? init[r2] : 0.0, a3 = init ? init[r3] : 0.0;
#pragma unroll 4
    for (int c = 0; c < cols; ++c) {
      const double xc = x(c);
      a0 = fma(w0[c], xc, a0);
      a1 = fma(w1[c], xc, a1);
      a2 = fma(w2[c], xc, a2);
      a3 = fma(w3[c], xc, a3);
    }
    out[r] = a0;
    if (r + 1 < rows) out[r + 1] = a1;
    if (r + 2 < rows) out[r + 2] = a2;
    if (r + 3 < rows) out[r + 3] = a3;
  }
}
// out[c] = sum_r Wm[r ldw + c] x[r], c < cols (the transposed product) -- four adjacent columns at a time
__device__ __forceinline__ void matvecT(const double* Wm, int ldw, int rows, int cols, const double* x, double* out) {
  for (int c = 0; c < cols; c += 4) {
    const int c1 = c + 1 < cols ? c + 1 : cols - 1, c2 = c + 2 < cols ? c + 2 : cols - 1, c3 = c + 3 < cols ? c + 3 : cols - 1;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
    for (int r = 0; r < rows; ++r) {
      const double xr = x[r];
      const double* w = Wm + (long)r * ldw;
      a0 = fma(w[c], xr, a0);
      a1 = fma(w[c1], xr, a1);
      a2 = fma(w[c2], xr, a2);
      a3 = fma(w[c3], xr, a3);
    }
    out[c] = a0;
    if (c + 1 < cols) out[c + 1] = a1;
    if (c + 2 < cols) out[c + 2] = a2;
    if (c + 3 < cols) out[c + 3] = a3;
  }
}

// F([x, t, y]) (src/model.py:153-156, 130-141); xproj[k] = Win[k, 0..d) x + Win.b[k] is hoisted (x does not move along a path)
// zs (or null): pre-activations of every layer, [m][GK], for the vector-Jacobian product
__device__ void field_eval(const Net& n, const double* xproj, double t, const double* y, double* out, double* zs) {
  const double* Win = n.th + n.o.Win;
  const int ld = n.o.ldin, K = n.K;
  double z[GK], z2[GK];
  for (int k = 0; k < K; ++k) z2[k] = fma(Win[k * ld + n.d], t, xproj[k]);
  matvec(Win + n.d + 1, ld, K, n.H, [&](int j) { return y[j]; }, z2, z);
  if (zs)
    for (int k = 0; k < K; ++k) zs[k] = z[k];
  for (int l = 1; l < n.m; ++l) {
    matvec(n.th + n.o.Wh, K, K, K, [&](int kk) { return z[kk] > 0.0 ? z[kk] : 0.0; }, n.th + n.o.Whb, z2);
    for (int k = 0; k < K; ++k) {
      z[k] = z2[k];
      if (zs) zs[l * GK + k] = z2[k];
    }
  }
  for (int k = 0; k < K; ++k) z[k] = xw_tanh(z[k]);
  matvec(n.th + n.o.Wo, K, n.H, K, [&](int k) { return z[k]; }, n.th + n.o.Wob, out);
}

// slab[e0 + i] += sum over the 16 paths of the group of term(i), i < n.  Sixteen entries at a time: every lane of the group ends
// up holding the total of ONE entry (a fixed butterfly of lane exchanges per entry) and the group adds them with one coalesced
// read-modify-write -- an entry is always touched by the same lane, in program order: deterministic, no atomics, and the memory
// round trip is paid once per 16 entries (per entry it was 0.5 us: 120 of the 150 ms of a sweep at (64, 16)).
template <class F>
__device__ __forceinline__ void gadd_run(double* slab, int e0, int n, bool active, F term) {
  const int l16 = threadIdx.x & 15;
  for (int c = 0; c < n; c += 16) {
    double mine = 0.0;
    for (int i = 0; i < 16; ++i) {
      if (c + i >= n) break;
      const double s_ = gsum16(active ? term(c + i) : 0.0);
      if (l16 == i) mine = s_;
    }
    if (c + l16 < n) slab[e0 + c + l16] += mine;
  }
}

// slab's read-out entries (FL_w, FL_b) for the output state y under the cotangent ub
__device__ __forceinline__ void path_readout_grad(double* slab, const Net& n, bool active, double ub, const double* y) {
  gadd_run(slab, n.o.FLw, n.H, active, [&](int h) { return ub * y[h]; });
  gadd_run(slab, n.o.FLb, 1, active, [&](int) { return ub; });
}

// a^T dF/d(y, theta) at (t, yin): gy[H] (overwritten), Sx[K] += cotangent of the input layer's pre-activation (the x columns and
// the bias of Win are contracted once per sweep from it), parameter gradients into the group's slab (or none: slab == null)
__device__ void field_vjp(const Net& n, const double* xproj, double t, const double* yin, const double* a, double* gy, double* Sx,
                          double* slab, bool active) {
  double zs[GM * GK], out[GH];
  field_eval(n, xproj, t, yin, out, zs);
  const int K = n.K, H = n.H, ld = n.o.ldin;
  const double* Wo = n.th + n.o.Wo;
  const double* Wh = n.th + n.o.Wh;
  const double* Win = n.th + n.o.Win;
  double dz[GK], dzp[GK], th[GK];
  for (int k = 0; k < K; ++k) th[k] = xw_tanh(zs[(n.m - 1) * GK + k]);
  matvecT(Wo, K, H, K, a, dz);
  for (int k = 0; k < K; ++k) dz[k] *= 1.0 - th[k] * th[k];
  if (slab) {
    for (int h = 0; h < H; ++h) {
      const double ah = a[h];
      gadd_run(slab, n.o.Wo + h * K, K, active, [&](int k) { return ah * th[k]; });
    }
    gadd_run(slab, n.o.Wob, H, active, [&](int h) { return a[h]; });
  }
  for (int l = n.m - 1; l >= 1; --l) {
    const double* zp = zs + (l - 1) * GK;
    if (slab) {
      for (int k = 0; k < K; ++k) {
        const double dk = dz[k];
        gadd_run(slab, n.o.Wh + k * K, K, active, [&](int kk) { return dk * (zp[kk] > 0.0 ? zp[kk] : 0.0); });
      }
      gadd_run(slab, n.o.Whb, K, active, [&](int k) { return dz[k]; });
    }
    matvecT(Wh, K, K, K, dz, dzp);
    for (int k = 0; k < K; ++k) dz[k] = zp[k] > 0.0 ? dzp[k] : 0.0;
  }
  if (slab) {
    for (int k = 0; k < K; ++k) {
      const double dk = dz[k];
      // columns d (the time) and d + 1 .. d + H (the state) of row k are contiguous
      gadd_run(slab, n.o.Win + k * ld + n.d, 1 + H, active, [&](int c) { return dk * (c == 0 ? t : yin[c - 1]); });
    }
  }
  for (int k = 0; k < K; ++k) Sx[k] += dz[k];
  matvecT(Win + n.d + 1, ld, K, H, dz, gy);
}

__device__ void lift(const Net& n, double s, double* pre0, double* pre2, double* y) {   // y0 = IL(start), src/model.py:78,97
  const double* th = n.th;
  const int H = n.H;
  for (int i = 0; i < H; ++i) pre0[i] = fma(th[n.o.IL0w + i], s, th[n.o.IL0b + i]);
  matvec(th + n.o.IL2w, H, H, H, [&](int j) { return pre0[j] > 0.0 ? pre0[j] : 0.0; }, th + n.o.IL2b, pre2);
  matvec(th + n.o.IL4w, H, H, H, [&](int j) { return pre2[j] > 0.0 ? pre2[j] : 0.0; }, th + n.o.IL4b, y);
}

__device__ void x_projection(const Net& n, const double* xT, int N, int path, double* xproj) {
  const double* Win = n.th + n.o.Win;
  for (int k = 0; k < n.K; ++k) {
    double acc = n.th[n.o.Winb + k];
    for (int i = 0; i < n.d; ++i) acc = fma(Win[k * n.o.ldin + i], xT[(long)i * N + path], acc);
    xproj[k] = acc;
  }
}
