// xw_disc_tiled.hip -- the TILED test-network family: v_phi (src/model.py:37-47) at the network's own width, 1 <= W <= 256,
// 0 <= q <= 32 tied hidden layers, every layer on v_mfma_f64_16x16x4.  Same semantics as xw_disc_fwd_xproj / xw_disc_bwd
// (include/xnwan.h), parameters in the plain blob layout v_offsets(d, W).
//
// Forward (k_dt_fwd): one wave per 8 points.  The 16 columns of a chain-layout tile (xw_common.h) are the 8 points' values a
// (columns 0..7) and their time tangents da (columns 8..15), so one weight fragment feeds both and every activation stays in
// registers from layer to layer: the D registers of layer j are the B registers of layer j + 1.  A column and its tangent sit
// 8 lanes apart; the tangent's ReLU gate reads its partner's value by a lane swap.  At W = 256 the input and output tiles are
// 2 x 64 doubles per lane.  Weight fragments are read from global memory (Vh is 512 KB at W = 256 and stays in L2).
// With gxv the wave keeps the ReLU masks of its layers in LDS and runs the reverse chain for the input gradient in the same
// columns (the tangent half then carries zeros).
//
// Record: relu(a_j) of the q tied layers and tanh(a_q), (q + 1) W doubles per point, in the containers' layout
// ([tile of 16 points][row j W + k][16]).
//
// Reverse (k_dt_bwd): one block of 4 waves per 64 points (one slab), 16 points per wave, grid-striding beyond 512 blocks.  Each
// wave runs the cotangent chain delta_j = mask_j (Vh^T delta_{j+1}) in registers; per layer the block posts delta_{j+1}
// transposed to LDS ([W][64 points]) and forms dVh += delta_{j+1} r_j^T with the contraction over the 64 points on the
// matrix unit (A from LDS, B straight from the record), one 16 x 16 tile of dVh per wave at a time, added into the block's
// own slab.  No float atomics: every slab entry has one writer and a fixed order.
#include <hip/hip_runtime.h>
#include "xw_disc_core.h"   // (the slab count of the reverse kernels: one function for every family)
#include "../../include/xnwan.h"

#define XWD_MAX_W 256
#define XWD_MAX_Q 32

namespace {

// record index of (row, point p)
__device__ __forceinline__ long dt_rec(long p, int rows, int row) { return ((p >> 4) * rows + row) * 16 + (p & 15); }

__device__ __forceinline__ double dt_swap8(double x) { return __shfl_xor(x, 8, 64); }

// forward: NT = row tiles of 16 held per lane (W <= 16 NT)
template <int NT>
__global__ void __launch_bounds__(256, 1) k_dt_fwd(const double* __restrict__ xT, const double* __restrict__ tf, const double* __restrict__ tpp,
                                                   const double* __restrict__ ph, int N, int L, int d, int W, int q,
                                                   double* __restrict__ v, double* __restrict__ vt, double* __restrict__ gxv,
                                                   double* __restrict__ gtv, int ngrad, double* __restrict__ act) {
  __shared__ unsigned long long sMask[4][XWD_MAX_Q][64];
  const int lane = xw_lane(), wave = threadIdx.x >> 6;
  const int n = lane & 15, g = lane >> 4, kind = n >> 3;
  const long P = (long)N * L;
  const long ntiles = (P + 7) / 8;
  const VOff o = v_offsets(d, W);
  const int rows = (q + 1) * W;
  const double* Vh = ph + o.Vh;
  for (long tile = (long)blockIdx.x * 4 + wave; tile < ntiles; tile += (long)gridDim.x * 4) {
    const long raw = tile * 8 + (n & 7);
    const bool valid = raw < P;
    const long p = valid ? raw : P - 1;
    double t;
    int nidx;
    xw_locate_pt(p, N, tf, tpp, t, nidx);
    const bool grad = gxv != nullptr && tile * 8 < ngrad;          // (wave-uniform)
    d4 a[NT], b[NT];
    // input layer: B rows = (t, x_0 .. x_{d-1}) for the values, e_0 for the tangents
#pragma unroll
    for (int ro = 0; ro < NT; ++ro) a[ro] = xw_zero4();
    for (int ks = 0; 4 * ks < d + 1; ++ks) {
      const int c = 4 * ks + g;
      double bin;
      if (kind) bin = c == 0 ? 1.0 : 0.0;
      else bin = c == 0 ? t : (c <= d ? xw_ld_g(xT + (long)(c - 1) * N + nidx) : 0.0);
#pragma unroll
      for (int ro = 0; ro < NT; ++ro)
        if (16 * ro < W) a[ro] = XW_MFMA(xw_fragA(ph + o.Vin, o.ldin, W, d + 1, 16 * ro, 4 * ks), bin, a[ro]);
    }
    if (!kind) {
#pragma unroll
      for (int ro = 0; ro < NT; ++ro) a[ro] += xw_vecD(ph + o.Vinb, W, 16 * ro);
    }
    for (int j = 0; j < q; ++j) {
      // ReLU in place (the tangent gated by its value's sign: relu'(0) = 0, as torch), record, mask
      unsigned long long mk = 0ull;
#pragma unroll
      for (int rt = 0; rt < NT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double x = a[rt][r];
          const double sw = dt_swap8(x);                             // (all lanes: the swap reads its partner's register)
          const double own = kind ? sw : x;
          const bool open = own > 0.0;
          a[rt][r] = open ? x : 0.0;
          if (open) mk |= 1ull << (rt * 4 + r);
          const int row = 16 * rt + g + 4 * r;
          if (act != nullptr && !kind && valid && row < W) xw_st_g(a[rt][r], act + dt_rec(p, rows, j * W + row));
        }
      if (grad) sMask[wave][j][lane] = mk;
#pragma unroll
      for (int ro = 0; ro < NT; ++ro) {
        if (16 * ro < W) b[ro] = kind ? xw_zero4() : xw_vecD(ph + o.Vhb, W, 16 * ro);
        else b[ro] = xw_zero4();
      }
#pragma unroll
      for (int ks = 0; ks < 4 * NT; ++ks) {
        if (4 * ks >= W) break;
        const double bin = a[ks >> 2][ks & 3];
#pragma unroll
        for (int ro = 0; ro < NT; ++ro)
          if (16 * ro < W) b[ro] = XW_MFMA(xw_fragA(Vh, W, W, W, 16 * ro, 4 * ks), bin, b[ro]);
      }
#pragma unroll
      for (int ro = 0; ro < NT; ++ro) a[ro] = b[ro];
    }
    // output layer: v = Vo tanh(a_q) + Vo.b,  dv/dt = Vo ((1 - tanh^2) da_q)
    double s = 0.0;
#pragma unroll
    for (int rt = 0; rt < NT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * rt + g + 4 * r;
        const double x = a[rt][r];
        const double sw = dt_swap8(x);
        const double th = xw_tanh(kind ? sw : x);
        const double vo = row < W ? xw_ld_g(ph + o.Vo + row) : 0.0;
        if (act != nullptr && !kind && valid && row < W) xw_st_g(th, act + dt_rec(p, rows, q * W + row));
        s = fma(vo, kind ? (1.0 - th * th) * x : th, s);
        b[rt][r] = kind ? 0.0 : vo * (1.0 - th * th);              // cotangent of a_q for the input gradient
      }
    s = xw_sum_over_g(s);
    if (valid && g == 0) {
      if (!kind) v[p] = s + ph[o.Vob];
      else if (vt != nullptr) vt[p] = s;
    }
    if (grad) {
      for (int j = q - 1; j >= 0; --j) {
        const unsigned long long mk = sMask[wave][j][lane];
#pragma unroll
        for (int ro = 0; ro < NT; ++ro) a[ro] = xw_zero4();
#pragma unroll
        for (int ks = 0; ks < 4 * NT; ++ks) {
          if (4 * ks >= W) break;
          const double bin = b[ks >> 2][ks & 3];
#pragma unroll
          for (int ro = 0; ro < NT; ++ro)
            if (16 * ro < W) a[ro] = XW_MFMA(xw_fragAT(Vh, W, W, W, 16 * ro, 4 * ks), bin, a[ro]);
        }
#pragma unroll
        for (int rt = 0; rt < NT; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) b[rt][r] = ((mk >> (rt * 4 + r)) & 1ull) ? a[rt][r] : 0.0;
      }
      // (t, x) rows of Vin^T delta_0
      for (int r0 = 0; r0 < d + 1; r0 += 16) {
        d4 acc = xw_zero4();
#pragma unroll
        for (int ks = 0; ks < 4 * NT; ++ks) {
          if (4 * ks >= W) break;
          acc = XW_MFMA(xw_fragAT(ph + o.Vin, o.ldin, W, d + 1, r0, 4 * ks), b[ks >> 2][ks & 3], acc);
        }
        if (!kind && raw < ngrad) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = r0 + g + 4 * r;
            if (row == 0) { if (gtv != nullptr) gtv[raw] = acc[r]; }
            else if (row <= d) gxv[(long)(row - 1) * ngrad + raw] = acc[r];
          }
        }
      }
    }
  }
}

// reverse from the record: slab blockIdx.x of gslab (zeroed here first) = the gradient of <vbar, v> over the block's points
#define XWD_LS 65                   // LDS row stride of the transposed cotangents [W][64 points]
template <int NT>
__global__ void __launch_bounds__(256, 1) k_dt_bwd(const double* __restrict__ xT, const double* __restrict__ tf, const double* __restrict__ tpp,
                                                   const double* __restrict__ ph, const double* __restrict__ vbar, int N, int L, int d,
                                                   int W, int q, const double* __restrict__ act, double* __restrict__ gslab) {
  __shared__ double sD[XWD_MAX_W * XWD_LS];
  const int lane = xw_lane(), wave = threadIdx.x >> 6, tid = threadIdx.x;
  const int n = lane & 15, g = lane >> 4;
  const long P = (long)N * L;
  const long nsuper = (P + 63) / 64;
  const VOff o = v_offsets(d, W);
  const int rows = (q + 1) * W;
  const double* Vh = ph + o.Vh;
  double* slab = gslab + (long)blockIdx.x * o.total;
  for (int i = tid; i < o.total; i += 256) slab[i] = 0.0;           // (the block's own slab: no memset node in front)
  __syncthreads();
  double accHb = 0.0, accIb = 0.0, accO = 0.0, accOb = 0.0;   // bias sums of thread tid (row tid), Vo[tid], Vo.b
  for (long st = blockIdx.x; st < nsuper; st += gridDim.x) {
    const long base = st * 64;
    const long raw = base + wave * 16 + n;
    const bool valid = raw < P;
    const long p = valid ? raw : P - 1;
    const double vb = valid ? (vbar != nullptr ? vbar[p] : 1.0) : 0.0;
    // output layer: delta_q = vbar Vo (1 - tanh^2)
    d4 dn[NT], dl[NT];
#pragma unroll
    for (int rt = 0; rt < NT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * rt + g + 4 * r;
        if (row < W) {
          const double th = xw_ld_g(act + dt_rec(p, rows, q * W + row));
          dn[rt][r] = vb * xw_ld_g(ph + o.Vo + row) * (1.0 - th * th);
        } else {
          dn[rt][r] = 0.0;
        }
      }
    if (tid < W) {
      for (int i = 0; i < 64; ++i) {
        const long pi = base + i;
        if (pi >= P) break;
        const double vbi = vbar != nullptr ? vbar[pi] : 1.0;
        accO = fma(vbi, xw_ld_g(act + dt_rec(pi, rows, q * W + tid)), accO);
        if (tid == 0) accOb += vbi;
      }
    }
    for (int j = q - 1; j >= -1; --j) {
      __syncthreads();                                             // (the previous layer's readers are done with sD)
#pragma unroll
      for (int rt = 0; rt < NT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * rt + g + 4 * r;
          if (row < W) sD[row * XWD_LS + wave * 16 + n] = dn[rt][r];
        }
      __syncthreads();
      if (tid < W) {
        double sb = 0.0;
        for (int i = 0; i < 64; ++i) sb += sD[tid * XWD_LS + i];
        if (j >= 0) accHb += sb; else accIb += sb;
      }
      if (j >= 0) {
        // dVh[k][kk] += sum over the 64 points of delta_{j+1}[k] r_j[kk]: wave w takes the column tiles kk0 = 16 (w + 4 i)
        for (int kt = wave; 16 * kt < W; kt += 4) {
          double bf[16];
#pragma unroll
          for (int ks = 0; ks < 16; ++ks) {
            const long pk = base + 4 * ks + g;
            const int col = 16 * kt + n;
            bf[ks] = (pk < P && col < W) ? xw_ld_g(act + dt_rec(pk, rows, j * W + col)) : 0.0;
          }
#pragma unroll
          for (int rt = 0; rt < NT; ++rt) {
            if (16 * rt >= W) break;
            d4 acc = xw_zero4();
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) acc = XW_MFMA(sD[(16 * rt + n) * XWD_LS + 4 * ks + g], bf[ks], acc);
            const int col = 16 * kt + n;
            if (col < W) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int row = 16 * rt + g + 4 * r;
                if (row < W) slab[o.Vh + row * W + col] += acc[r];
              }
            }
          }
        }
        // delta_j = (r_j > 0) (Vh^T delta_{j+1})
#pragma unroll
        for (int ro = 0; ro < NT; ++ro) dl[ro] = xw_zero4();
#pragma unroll
        for (int ks = 0; ks < 4 * NT; ++ks) {
          if (4 * ks >= W) break;
          const double bin = dn[ks >> 2][ks & 3];
#pragma unroll
          for (int ro = 0; ro < NT; ++ro)
            if (16 * ro < W) dl[ro] = XW_MFMA(xw_fragAT(Vh, W, W, W, 16 * ro, 4 * ks), bin, dl[ro]);
        }
#pragma unroll
        for (int rt = 0; rt < NT; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * rt + g + 4 * r;
            const double rj = row < W ? xw_ld_g(act + dt_rec(p, rows, j * W + row)) : 0.0;
            dn[rt][r] = rj > 0.0 ? dl[rt][r] : 0.0;
          }
      } else {
        // dVin[k][c] += sum over the points of delta_0[k] (t, x)[c]: wave w takes the column tiles 16 (w + 4 i) of the d + 1
        for (int kt = wave; 16 * kt < d + 1; kt += 4) {
          double bf[16];
#pragma unroll
          for (int ks = 0; ks < 16; ++ks) {
            const long pk = base + 4 * ks + g;
            const int col = 16 * kt + n;
            double val = 0.0;
            if (pk < P && col <= d) {
              double tk;
              int nk;
              xw_locate_pt(pk, N, tf, tpp, tk, nk);
              val = col == 0 ? tk : xw_ld_g(xT + (long)(col - 1) * N + nk);
            }
            bf[ks] = val;
          }
#pragma unroll
          for (int rt = 0; rt < NT; ++rt) {
            if (16 * rt >= W) break;
            d4 acc = xw_zero4();
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) acc = XW_MFMA(sD[(16 * rt + n) * XWD_LS + 4 * ks + g], bf[ks], acc);
            const int col = 16 * kt + n;
            if (col <= d) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int row = 16 * rt + g + 4 * r;
                if (row < W) slab[o.Vin + row * o.ldin + col] += acc[r];
              }
            }
          }
        }
      }
    }
  }
  // (only blocks that took a super-tile reach here with non-zero sums; the others add zeros to their zeroed slab)
  if (tid < W) {
    slab[o.Vhb + tid] += accHb;
    slab[o.Vinb + tid] += accIb;
    slab[o.Vo + tid] += accO;
  }
  if (tid == 0) slab[o.Vob] += accOb;
}

}  // namespace

extern "C" int xw_disc_tiled_ok(int d, int W, int q) {
  return W >= 1 && W <= XWD_MAX_W && q >= 0 && q <= XWD_MAX_Q && d >= 1 && d + 2 <= 128;
}

extern "C" int xw_disc_tiled_act_rows(int W, int q) { return xw_disc_tiled_ok(1, W, q) ? (q + 1) * W : XW_E_DIMS; }

#define XWD_DISPATCH(KERNEL, GRID, ...)                                                                                    \
  do {                                                                                                                    \
    if (W <= 64) hipLaunchKernelGGL(KERNEL<4>, dim3(GRID), dim3(256), 0, s, __VA_ARGS__);                                 \
    else if (W <= 128) hipLaunchKernelGGL(KERNEL<8>, dim3(GRID), dim3(256), 0, s, __VA_ARGS__);                           \
    else if (W <= 192) hipLaunchKernelGGL(KERNEL<12>, dim3(GRID), dim3(256), 0, s, __VA_ARGS__);                          \
    else hipLaunchKernelGGL(KERNEL<16>, dim3(GRID), dim3(256), 0, s, __VA_ARGS__);                                        \
  } while (0)

extern "C" int xw_disc_tiled_fwd(const double* xT, const double* t, const double* tpp, const double* phi, int N, int L, int d,
                                 int W, int q, double* v, double* vt, double* gxv, double* gtv, int ngrad, int max_blocks,
                                 double* act, const double* xproj, void* stream) {
  if (!xT || !phi || !v || N <= 0 || L <= 0 || d <= 0 || q < 0 || W <= 0 || xproj != nullptr) return XW_E_ARG;
  if (!tpp && !t) return XW_E_ARG;
  if (tpp && L != 1) return XW_E_ARG;
  if (gxv && (ngrad <= 0 || (long)ngrad > (long)N * L)) return XW_E_ARG;
  if (!xw_disc_tiled_ok(d, W, q)) return XW_E_DIMS;
  const long P = (long)N * L;
  if (P * (q + 1) * W >= (1L << 40)) return XW_E_ARG;
  long blocks = (P + 31) / 32;                                 // 4 waves of 8 points
  const long cap = max_blocks > 0 ? max_blocks : 1024;
  if (blocks > cap) blocks = cap;
  hipStream_t s = (hipStream_t)stream;
  XWD_DISPATCH(k_dt_fwd, (unsigned)blocks, xT, t, tpp, phi, N, L, d, W, q, v, vt, gxv, gtv, ngrad, act);
  return xw_launch_status();
}

extern "C" int xw_disc_tiled_bwd(const double* xT, const double* t, const double* tpp, const double* phi, const double* vbar,
                                 int N, int L, int d, int W, int q, const double* act, double* gslab, void* stream) {
  if (!xT || !phi || !gslab || N <= 0 || L <= 0 || d <= 0 || q < 0 || W <= 0) return XW_E_ARG;
  if (!tpp && !t) return XW_E_ARG;
  if (tpp && L != 1) return XW_E_ARG;
  if (!xw_disc_tiled_ok(d, W, q)) return XW_E_DIMS;
  if (!act) return XW_E_DIMS;                                  // (from the record only)
  const long P = (long)N * L;
  const int nslab = bwd_blocks(P);
  hipStream_t s = (hipStream_t)stream;
  XWD_DISPATCH(k_dt_bwd, (unsigned)nslab, xT, t, tpp, phi, vbar, N, L, d, W, q, act, gslab);
  return xw_launch_status();
}
