// xw_ode_core.h -- XNODE primal network u_theta on gfx950: the fused fixed-grid ODE stepper, what its forward pass and its reverse
// sweeps share.
//
// The stepper replaces NeuralODE.forward + _F/_ODEField + torchdiffeq's Python stepping loop (src/model.py:87-112,140-156 of the
// reference) and the autograd replay of that loop (src/loss.py:55, src/training.py:137).
//
// One wave = 16 Monte-Carlo paths.  The hidden state y[H], the field's pre-activations z_j[K] and every cotangent live
// in registers in the "chain layout" of xw_common.h for the whole time loop; all weight matrices are MFMA A-fragments
// held in registers (13 + 14 f64 per lane at H=20, K=10).  Per field evaluation: 5 + 3(m-1) + 6 MFMAs forward and the
// same number for the vector-Jacobian product; parameter gradients are contractions over the 16 paths, done as 4-step
// MFMA outer products after an LDS transpose (xw_writeT / xw_readT), accumulated in registers over all stages, layers
// and time steps and written once per wave as a deterministic partial "slab".
//
// Memory traffic per path: x (d floats) once, the checkpoint y[L,H] written once / read once, u[L] -- everything else
// stays on chip.  At the headline size this kernel is bound by the FP64 matrix pipe, not by HBM.
//
// The layout, one source per kernel group (Makefile: two objects per width, xw_ode.hip with xw_ode_fwd.h in front of it, and xw_ode.hip's
// recomputing sweeps on their own):
//   xw_ode_core.h    this file: tableaux, Dim, Save / SaveX, the sinks, outer products, lift, project_x, the job tables, the cotangent
//                    forms, the activation store, the slab stores, sweep_tail (the 16-path and the narrow-tile sweeps end with it), the kernel tables' builder
//   xw_ode_select.h  which kernel a launch lands on: pure host functions
//   xw_ode_fwd.h     k_ode_fwd, the forward table, xw_ode_fwd_multi_w
//   xw_ode.hip       sweep_body, k_ode_bwd, k_ode_bwd_duo, the sweep table, xw_ode_bwd_multi_w | xw_ode_bwd_recomp_w
// What depends on the matrix instruction the FIELD runs on is one of two headers, included once (-DXW_ODE_WIDE16 chooses, in the two sources):
//   xw_ode_mfma4.h   v_mfma_f64_4x4x4    the narrow containers (20, 10) and (32, 12), with the narrow tiles of xw_ode_n4.h
//   xw_ode_mfma16.h  v_mfma_f64_16x16x4  the wide container (64, 16)
// Every kernel, FwdJobs and BwdJobs stay in the anonymous namespace: they are part of the kernels' symbols.
#pragma once
#include <array>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include "xw_common.h"
#ifndef XW_ODE_FWD_WAVES
#define XW_ODE_FWD_WAVES 2     // waves per SIMD the forward pass's register allocation leaves room for (2: <= 256 registers; 3: <= 168)
#endif
#include "xnwan.h"

// One object per stepper width (Makefile: -DXW_ODE_H=.. -DXW_ODE_K=..), every depth m = 1..10 in it; the public entry
// points live in xw_ode_abi.hip and pick the object by (H, K).  Narrower networks run zero-padded inside the next larger
// width (exact: padding units stay identically zero, nets.Blob).
#if !defined(XW_ODE_H) || !defined(XW_ODE_K)
#error "compile with -DXW_ODE_H=<u_hidden_dim> -DXW_ODE_K=<u_hidden_hidden_dim>"
#endif
#define XW_CAT4_(a, b, c, d) a##b##c##d
#define XW_CAT4(a, b, c, d) XW_CAT4_(a, b, c, d)
#define XW_ODE_FN(name) XW_CAT4(name, XW_ODE_H, _, XW_ODE_K)
#include "xw_ode_select.h"
static_assert(XW_ODE_DEPTHS == XW_ODE_MAX_LAYERS, "the depths of the kernel tables");

namespace {

// ---- explicit Runge-Kutta tableaux of the fixed-grid solvers (torchdiffeq fixed_grid: euler, midpoint, rk4 = 3/8 rule)
template <int METHOD> struct RK;
template <> struct RK<0> {
  static constexpr int S = 1;
  __device__ static constexpr double c(int) { return 0.0; }
  __device__ static constexpr double a(int, int) { return 0.0; }
  __device__ static constexpr double b(int) { return 1.0; }
};
template <> struct RK<1> {
  static constexpr int S = 2;
  __device__ static constexpr double c(int i) { return i == 1 ? 0.5 : 0.0; }
  __device__ static constexpr double a(int i, int j) { return (i == 1 && j == 0) ? 0.5 : 0.0; }
  __device__ static constexpr double b(int i) { return i == 1 ? 1.0 : 0.0; }
};
template <> struct RK<2> {
  static constexpr int S = 4;
  __device__ static constexpr double c(int i) { return i == 1 ? 1.0 / 3.0 : i == 2 ? 2.0 / 3.0 : i == 3 ? 1.0 : 0.0; }
  __device__ static constexpr double a(int i, int j) {
    return (i == 1 && j == 0) ? 1.0 / 3.0
         : (i == 2 && j == 0) ? -1.0 / 3.0
         : (i == 2 && j == 1) ? 1.0
         : (i == 3 && j == 0) ? 1.0
         : (i == 3 && j == 1) ? -1.0
         : (i == 3 && j == 2) ? 1.0 : 0.0;
  }
  __device__ static constexpr double b(int i) { return (i == 0 || i == 3) ? 0.125 : 0.375; }
};

template <int H, int K> struct Dim {
  static constexpr int HT = (H + 15) / 16;   // row tiles of an H-vector
  static constexpr int KSH = (H + 3) / 4;    // k-steps of a contraction over H
  static constexpr int KSK = (K + 3) / 4;    // k-steps of a contraction over K
  static constexpr int KR = (K + 1 + 3) / 4;   // live registers of a K-tile incl. the ones row (rows 0 .. K)
  static constexpr int KB = (K + 3) / 4;     // 4-row blocks of a K-vector (= live registers of its chain tile)
  static constexpr int HB = (H + 3) / 4;     // 4-row blocks of an H-vector
  __device__ static constexpr int HR(int ht) { return (H - 16 * ht) >= 16 ? 4 : (H - 16 * ht + 3) / 4; }        // rows of y
  __device__ static constexpr int HR1(int ct) { return (H + 1 - 16 * ct) >= 16 ? 4 : (H + 1 - 16 * ct + 3) / 4; }  // + time row
  static constexpr int CT = (H + 16) / 16;   // 16-row tiles of [y ; t]: the time row H is its own tile when H % 16 == 0
};

template <int M> struct Save {               // what the VJP of one field evaluation needs
  d4 z[M > 1 ? M - 1 : 1];                   // relu(z_0) .. relu(z_{m-2}): layer inputs; their sign pattern is the ReLU mask
  d4 a;                                      // tanh(z_{m-1})
  __device__ __forceinline__ bool pos(int j, int r) const { return z[j][r] > 0.0; }
  __device__ __forceinline__ double gate(int j, int r, double x) const { return z[j][r] > 0.0 ? x : 0.0; }   // relu'(z_j) * x
};
// the same for a sweep without weight gradients: the layer inputs are only needed as their ReLU masks, one bit per live
// register of the K-tile and layer in one word -- the x-only sweep then loads 1 word + tanh instead of m K doubles per stage.
// The forward pushes the bit (z > 0) of every pre-activation register into the word as it is produced (a compare and one
// add-with-carry: word = word + word + carry): (layer j, register r) was push number XW_KB j + r of XW_KB (M - 1) and sits
// at bit  XW_KB (M - 1) - 1 - (XW_KB j + r).  The test must be z > 0, not the sign bit: a layer whose units are all dead
// feeds EXACT zeros (+0, the biases start at zero) to the next one, and relu'(+0) = 0 in the reference (torch) -- with sign
// bits the boundary sweep of the d = 20 fixture was off by 5e-5.
#define XW_KB ((XW_ODE_K + 3) / 4)
// (more than 32 bits -- the wide container, 4 (m - 1) bits per stage, at depth 10: 36 -- take a second word, bits_hi = bits 32 and up; XW_MASK_WORDS)
#define XW_MASK_WORDS(M) ((XW_KB * ((M) - 1) > 32) ? 2 : 1)
template <int M> struct SaveX {
  static_assert(XW_KB * (M - 1) <= 64, "mask words");
  d4 a;
  unsigned bits, bits_hi;
  __device__ static constexpr int bit(int j, int r) { return XW_KB * (M - 1) - 1 - (XW_KB * j + r); }
  __device__ __forceinline__ bool pos(int j, int r) const { return ((bit(j, r) < 32 ? bits >> bit(j, r) : bits_hi >> (bit(j, r) - 32)) & 1u) != 0; }
  // relu'(z_j) * x as two 32-bit ANDs with the mask bit spread to 0 / ~0 (one v_bfe_i32 that does not depend on x):
  // a v_cndmask_b32 costs ~6 clocks of the SIMD, a v_and_b32 2.3 (profiles/r02_probe_coexec.txt), and the gate sits on the
  // adjoint chain's critical path once per layer and register
  __device__ __forceinline__ double gate(int j, int r, double x) const {
    const int m = bit(j, r) < 32 ? __builtin_amdgcn_sbfe((int)bits, bit(j, r), 1) : __builtin_amdgcn_sbfe((int)bits_hi, bit(j, r) - 32, 1);
    return __hiloint2double(__double2hiint(x) & m, __double2loint(x) & m);
  }
};

// F([x, t, y]) of src/model.py:153-156 (field_fwd of the form header): z0 = Win [x;t;y] + b (x part pre-contracted into xp),
// (m-1) tied ReLU layers, tanh, output layer.  y/out: HT chain tiles.
// Where the layer inputs of an evaluation go: nowhere, into registers (Save), or straight to the activation store.
struct SinkNone {
  __device__ __forceinline__ void fence() const {}
  __device__ __forceinline__ double relu(int, int, double z) const { return xw_relu1(z); }
  __device__ __forceinline__ void z(int, d4) const {}
  __device__ __forceinline__ void a(d4) const {}
};
template <int M> struct SinkSave {
  Save<M>& sv;
  __device__ __forceinline__ void fence() const {}
  __device__ __forceinline__ double relu(int, int, double z) const { return xw_relu1(z); }
  __device__ __forceinline__ void z(int j, d4 r) const { sv.z[j] = r; }
  __device__ __forceinline__ void a(d4 v) const { sv.a = v; }
};

// D[i][j] += sum over the 16 paths of Q[i][path] * R[j][path]
// The block is exactly ONE wave and the LDS executes a wave's DS instructions in issue order, so the transposing
// write -> read round trip needs no s_barrier: a compiler-level fence keeps the program order of the accesses.
// QR / RR: live registers (4-row groups) of the two tiles
template <int QR = 4, int RR = 4>
__device__ __forceinline__ void outer_acc(d4& acc, d4 q, d4 r, double* lds) {
  xw_writeT_n<QR>(lds, q);
  xw_writeT_n<RR>(lds + XW_TTILE, r);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) acc = XW_MFMA(xw_readT(lds, ks), xw_readT(lds + XW_TTILE, ks), acc);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
// elementwise helpers on the first nr registers of a tile (nr is a compile-time constant after unrolling): an H-vector's
// last tile has H - 16 live rows, the rest is padding that no MFMA ever reads -- on this chip every FP64 VALU
// instruction of the lone sweep wave is time the matrix pipe stands still.
__device__ __forceinline__ void t_axpy(d4& y, double a, const d4& x, int nr) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (r < nr) y[r] += a * x[r];
}
__device__ __forceinline__ void t_scale(d4& y, double a, const d4& x, int nr) {
#pragma unroll
  for (int r = 0; r < 4; ++r) y[r] = r < nr ? a * x[r] : 0.0;
}
__device__ __forceinline__ void t_add(d4& y, const d4& x, int nr) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (r < nr) y[r] += x[r];
}
// Outer product whose R operand is a K-row activation followed by a row of ones (the bias gradient rides along as column
// K of the accumulator).  The ones row lives permanently in a dedicated LDS tile (written once per kernel): only the K
// real rows are stored, nothing is patched into registers.
template <int QR, int K>
__device__ __forceinline__ void outer_acc_ones(d4& acc, d4 q, d4 r, double* lds) {
  double* rt = lds + 2 * XW_TTILE;
  xw_writeT_n<QR>(lds, q);
  {
    const int l = xw_lane();
    const int g = l >> 4, n = l & 15;
#pragma unroll
    for (int rr = 0; rr < (K + 3) / 4; ++rr)
      if (4 * rr + 3 < K || g + 4 * rr < K) rt[(g + 4 * rr) * XW_TSTRIDE + n] = r[rr];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) acc = XW_MFMA(xw_readT(lds, ks), xw_readT(rt, ks), acc);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
// set chain-layout row `row` (0..15) of a tile to the value v in every column
__device__ __forceinline__ void set_row(d4& q, int row, double v) {
  if ((xw_lane() >> 4) == (row & 3)) q[row >> 2] = v;
}

// The two halves of an outer product, so that the chain's next matrix instructions can be issued between the LDS
// stores and the loads that read them back transposed: the lone wave has nothing else to cover that round trip with.
template <int QR, int RR>
__device__ __forceinline__ void outer_post(d4 q, d4 r, double* lds) {                 // general R tile
  xw_writeT_n<QR>(lds, q);
  xw_writeT_n<RR>(lds + XW_TTILE, r);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_sched_barrier(0);
}
template <int QR, int K>
__device__ __forceinline__ void outer_post_ones(d4 q, d4 r, double* lds) {            // K rows + the permanent ones row
  double* rt = lds + 2 * XW_TTILE;
  xw_writeT_n<QR>(lds, q);
  const int l = xw_lane();
  const int g = l >> 4, n = l & 15;
#pragma unroll
  for (int rr = 0; rr < (K + 3) / 4; ++rr)
    if (4 * rr + 3 < K || g + 4 * rr < K) rt[(g + 4 * rr) * XW_TSTRIDE + n] = r[rr];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_sched_barrier(0);
}
// The operand loads of an outer product are issued right behind its stores (the LDS executes one wave's accesses in
// order) and BEFORE the chain's next matrix instructions, the four accumulating MFMAs after them: with the 18-clock
// 4x4x4 chain a layer's 9 instructions no longer cover a store -> load -> use round trip started behind them (the sweep
// with weight gradients stood at 209 us where the chain alone had gained 30 %).
struct OuterOps { double a[4], b[4]; };
__device__ __forceinline__ void outer_fetch(OuterOps& o, const double* qt, const double* rt) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    o.a[ks] = xw_readT(qt, ks);
    o.b[ks] = xw_readT(rt, ks);
  }
  __builtin_amdgcn_sched_barrier(0);
}
// operands of two products that share one side (two row tiles against one R tile, or one Q tile against two R tiles)
__device__ __forceinline__ void outer_fetch1(double (&x)[4], const double* t) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) x[ks] = xw_readT(t, ks);
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void outer_fire(d4& acc, const double (&a)[4], const double (&b)[4]) {
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) acc = XW_MFMA(a[ks], b[ks], acc);
  __builtin_amdgcn_sched_barrier(0);
}
// LDS plan of a sweep block (one wave): tiles of XW_TTILE doubles
//   0 Q | 1 R | 2 R of K rows + a permanent row of ones | 3 second Q (last H row tile) | 4, 5 further R tiles of [y ; t]
#define XW_SWEEP_TILES 6
// start scalar -> hidden state: initial_layers of src/model.py:78,97
template <int H, int K>
__device__ __forceinline__ void lift(const double* __restrict__ th, const UOff& o, double sv, d4 (&a0)[Dim<H, K>::HT],
                                     d4 (&a1)[Dim<H, K>::HT], d4 (&y)[Dim<H, K>::HT]) {
  typedef Dim<H, K> D;
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht)
    a0[ht] = xw_relu(xw_vecD(th + o.IL0w, H, 16 * ht) * sv + xw_vecD(th + o.IL0b, H, 16 * ht));
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) {
    d4 v = xw_vecD(th + o.IL2b, H, 16 * ht);
#pragma unroll
    for (int ks = 0; ks < D::KSH; ++ks) v = XW_MFMA(xw_fragA(th + o.IL2w, H, H, H, 16 * ht, 4 * ks), a0[ks >> 2][ks & 3], v);
    a1[ht] = xw_relu(v);
  }
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) {
    d4 v = xw_vecD(th + o.IL4b, H, 16 * ht);
#pragma unroll
    for (int ks = 0; ks < D::KSH; ++ks) v = XW_MFMA(xw_fragA(th + o.IL4w, H, H, H, 16 * ht, 4 * ks), a1[ks >> 2][ks & 3], v);
    y[ht] = v;
  }
}

// xp = Win.b + Win[:, :d] x   (time-invariant along a path: src/model.py:99,154)
template <int H, int K>
__device__ __forceinline__ d4 project_x(const double* __restrict__ th, const UOff& o, const double* __restrict__ xT,
                                        int N, int d, int ncl) {
  const int g = xw_lane() >> 4;
  d4 xp = xw_vecD(th + o.Winb, K, 0);
  for (int ks = 0; ks < (d + 3) / 4; ++ks) {
    const int i = 4 * ks + g;
    const double b = i < d ? xT[(long)i * N + ncl] : 0.0;
    xp = XW_MFMA(xw_fragA(th + o.Win, o.ldin, K, d, 0, 4 * ks), b, xp);
  }
  return xp;
}

// Up to XW_MAXJOBS independent groups of paths (e.g. interior + boundary sample, or two cotangents of the same sample)
// run in ONE launch: one wave per 16 paths only fills a quarter of the chip at N = 4096, and separate launches on
// separate streams do not reliably overlap (they can land on the same hardware queue).
#define XW_MAXJOBS 4
struct FwdJobs {
  const double* xT[XW_MAXJOBS];
  const double* start[XW_MAXJOBS];
  double* u[XW_MAXJOBS];
  double* Y[XW_MAXJOBS];
  double* act[XW_MAXJOBS];     // optional: stage activations of every step (ActLayout), read back by the sweeps
  int N[XW_MAXJOBS];
  int tile0[XW_MAXJOBS + 1];   // first block of each job
  int n;
  int x_only;                  // the stores of this launch only serve x-only sweeps (XwOdeFwdJob.act_x_only)
  int narrow;                  // narrow tiles (XwOdeFwdJob.narrow, xw_ode_n4.h)
  int prio;                    // wave priority (XW_ODE_PRIO - XwOdeFwdJob.prio_drop)
  double* zero16;              // optional: 16 doubles cleared by block 0 (the sub-step's partial-sum slots)
};
struct BwdJobs {
  const double* xT[XW_MAXJOBS];
  const double* start[XW_MAXJOBS];
  const double* Y[XW_MAXJOBS];
  const double* act[XW_MAXJOBS];
  const double* ubar[XW_MAXJOBS];
  double* gx[XW_MAXJOBS];
  double* gs[XW_MAXJOBS];
  double* gslab[XW_MAXJOBS];
  int N[XW_MAXJOBS];
  int tile0[XW_MAXJOBS + 1];
  int n;
  int x_ones;                  // gx, gs are those of the all-ones cotangent (ubar == 1 at every time index >= 1)
  int prio;                    // wave priority of this launch: XW_ODE_PRIO unless mode bits 5..6 lower it (XW_ODE_PRIO - bits)
  int spread;                  // duo sweep: spacer rounds of this many blocks between the rounds of tiles (k_ode_bwd_duo), 0 = none
  // cotangent from a residual (XwOdeBwdJob.res_*): ubar[l][n] = base + coef (res_u[l][n] - ref)
  const double* res_u[XW_MAXJOBS];
  const double* res_ref[XW_MAXJOBS];
  double res_coef[XW_MAXJOBS], res_base[XW_MAXJOBS];
  int res_first[XW_MAXJOBS];        // XwOdeBwdJob.res_first_only: 0 / 1 residual forms, 2 = the weak form's dI/du, 3 = merged (1 + s * 2)
  const double* res_w[XW_MAXJOBS];
  const double* res_c[XW_MAXJOBS];
  const double* res_cp[XW_MAXJOBS];
  double res_kappa2[XW_MAXJOBS];
  int res_wpp[XW_MAXJOBS];
  // kind 3 (merged): kind 1 with these fields + (2 / res_scal[0]) kind 2 with the ones above
  const double* res_scal[XW_MAXJOBS];
  const double* res_refA[XW_MAXJOBS];
  double res_coefA[XW_MAXJOBS], res_baseA[XW_MAXJOBS];
};
// cotangent of u at (time index l, path col) of job `job`: a stored array, all ones, or formed from a residual on the fly
// (the initial-value and the boundary penalty: no cotangent kernel between the forward pass and these sweeps)
__device__ __forceinline__ double cot_u(const BwdJobs& jobs, int job, const double* __restrict__ ubar, int l, int N, int col,
                                        int L) {
  const double* __restrict__ ru = jobs.res_u[job];
  if (ru != nullptr) {
    if (jobs.res_first[job] >= 2) {
      // dI/du of the weak form (xw_gen_cotangents' basis B, src/loss.py:64,70): coef d(c(u) u)/du v w, + base v at t_{L-1}
      const long p = (long)l * N + col;
      const double ul = ru[p], vl = jobs.res_ref[job][p];
      const double wl = jobs.res_wpp[job] ? jobs.res_w[job][p] : jobs.res_w[job][col];
      const double dcu = jobs.res_c[job] != nullptr ? jobs.res_c[job][p] + ul * jobs.res_cp[job][p] : jobs.res_kappa2[job] * ul;
      const double gB = xw_cot_weak(jobs.res_coef[job], jobs.res_base[job], dcu, vl, wl, l == L - 1);
      if (jobs.res_first[job] == 2) return gB;
      // merged (xw_gen_cotangents with scal): pollution + the initial penalty at t_0, + (2 / I) dI/du
      return xw_cot_merged(xw_cot_init(jobs.res_baseA[job], jobs.res_coefA[job], ul, jobs.res_refA[job][col], l == 0),
                           2.0 / jobs.res_scal[job][0], gB);
    }
    if (jobs.res_first[job]) return xw_cot_init(jobs.res_base[job], jobs.res_coef[job], ru[col], jobs.res_ref[job][col], l == 0);
    double r = jobs.res_base[job];
    r += jobs.res_coef[job] * (ru[(long)l * N + col] - jobs.res_ref[job][(long)l * N + col]);
    return r;
  }
  return ubar != nullptr ? ubar[(long)l * N + col] : 1.0;
}
// ---- cotangent of u, one step ahead and without a branch around a load -------------------------------------------------
// cot_u() above branches on the kind of cotangent, and a value loaded inside a branch is used inside it: the
// wait in front of that use is vmcnt(0) -- it would drain the stage records this wave has just requested for the NEXT stage,
// i.e. expose a full memory latency in every step of a chain that is only ~2 - 4 k clocks long.  Here every kind is the same
// straight-line code: up to six loads from lane pointers prepared once (a pointer that a kind does not need aims at res_u /
// Y, finite data; its value is dropped by a select, never multiplied in), issued a whole step before their use.
//   affine kinds:  ub = cb + [st] + coef (ru - rf) [only at l = 0 when `first`]        (ones / stored / residual forms)
//   weak kind   :  ub = coef d(c u)/du v w  (+ base v at l = L - 1),  d(c u)/du = c + u c' (tabulated) or kappa2 u
//   merged kind :  ub = [baseA + coefA (u - h) at l = 0] + s (weak kind),  s = 2 / I read ONCE here, in front of the time
//                  loop; a sixth load (h, stride 0) rides in the weak kind's request, dropped by a select when not merged
struct Cot4 {
  const double *p0, *p1, *p2, *p3, *p4, *p5; // st | ru, rf | (weak) u, v, w, c, c', h   lane pointers at time index 0
  long s0, s1, s2;                           // strides (doubles) per time index of p0, (p1, p2 | p3, p4), p2 of the weak kind
  double cb, coef, base, kappa2, s, coefA, baseA;
  bool weak, use_st, use_res, first, tab, valid, merged;
};
struct CotRaw { double a, b, c, d, e, f; };
__device__ __forceinline__ Cot4 make_cot(const BwdJobs& jobs, int job, int N, int col, bool valid, const double* dummy) {
  Cot4 c;
  const double* ru = jobs.res_u[job];
  const double* ubar = jobs.ubar[job];
  c.valid = valid;
  c.weak = ru != nullptr && jobs.res_first[job] >= 2;
  c.merged = ru != nullptr && jobs.res_first[job] == 3;
  c.coefA = jobs.res_coefA[job];
  c.baseA = jobs.res_baseA[job];
  // One load and one FP64 divide per wave, in front of the time loop, for EVERY kind (no branch around a load): the kinds that
  // are not merged read Y[0] and drop the quotient by a select.  The weak kinds (2, 3) also carry the sixth load per step, h for
  // kind 3, Y[col] (stride 0, a cache hit after the first step) for kind 2.  What that costs the sweeps that gained nothing --
  // x-only, boundary, kind 2 alone -- has not been measured; tools/kernel_times.py prints those launches.
  c.s = 2.0 / xw_ld_g(c.merged ? jobs.res_scal[job] : dummy);       // (not merged: finite or not, dropped by the select)
  c.p5 = (c.merged ? jobs.res_refA[job] : dummy) + col;
  c.use_res = ru != nullptr && !c.weak;
  c.use_st = ru == nullptr && ubar != nullptr;
  c.first = c.use_res && jobs.res_first[job] != 0;
  c.cb = ru != nullptr ? jobs.res_base[job] : (ubar != nullptr ? 0.0 : 1.0);
  c.coef = jobs.res_coef[job];
  c.base = jobs.res_base[job];
  c.kappa2 = jobs.res_kappa2[job];
  c.tab = c.weak && jobs.res_c[job] != nullptr;
  if (c.weak) {
    c.p0 = ru + col; c.p1 = jobs.res_ref[job] + col; c.p2 = jobs.res_w[job] + col;
    c.p3 = (c.tab ? jobs.res_c[job] : ru) + col; c.p4 = (c.tab ? jobs.res_cp[job] : ru) + col;
    c.s0 = N; c.s1 = N; c.s2 = jobs.res_wpp[job] ? N : 0;
  } else {
    c.p0 = (c.use_st ? ubar : dummy) + col; c.s0 = c.use_st ? N : 0;
    c.p1 = (c.use_res ? ru : dummy) + col; c.p2 = (c.use_res ? jobs.res_ref[job] : dummy) + col;
    c.s1 = (c.use_res && !c.first) ? N : 0; c.s2 = 0;
    c.p3 = c.p4 = dummy;
  }
  return c;
}
template <bool WEAK> __device__ __forceinline__ CotRaw cot_issue(const Cot4& c, int l) {
  CotRaw r;
  r.a = xw_ld_g(c.p0 + l * c.s0);
  r.b = xw_ld_g(c.p1 + l * c.s1);
  if (WEAK) {
    r.c = xw_ld_g(c.p2 + l * c.s2);
    r.d = xw_ld_g(c.p3 + l * c.s1);
    r.e = xw_ld_g(c.p4 + l * c.s1);
    r.f = xw_ld_g(c.p5);
  } else {
    r.c = xw_ld_g(c.p2 + l * c.s1);
    r.d = r.e = r.f = 0.0;
  }
  return r;
}
template <bool WEAK> __device__ __forceinline__ double cot_value(const Cot4& c, const CotRaw& r, int l, int L) {
  double ub;
  if (WEAK) {
    const double dcu = c.tab ? fma(r.a, r.e, r.d) : c.kappa2 * r.a;        // (as cot_u: c + u c', or kappa2 u)
    ub = xw_cot_weak(c.coef, c.base, dcu, r.b, r.c, l == L - 1);
    if (c.merged) ub = xw_cot_merged(xw_cot_init(c.baseA, c.coefA, r.a, r.f, l == 0), c.s, ub);
  } else if (c.first) {
    ub = xw_cot_init(c.cb, c.coef, r.b, r.c, l == 0);
  } else {
    ub = c.cb;
    if (c.use_st) ub += r.a;
    if (c.use_res) ub = fma(c.coef, r.b - r.c, ub);
  }
  return c.valid ? ub : 0.0;
}

// vb: the 16-path tile of the launch this wave works on (= blockIdx.x in the one-tile-per-block kernels)
template <typename J> __device__ __forceinline__ int find_job(const J& jobs, int vb) {
  int j = 0;
#pragma unroll
  for (int k = 1; k < XW_MAXJOBS; ++k)
    if (k < jobs.n && vb >= jobs.tile0[k]) j = k;
  return j;
}

// The stepper's waves are latency chains that share their SIMD with a wave of the test network in the first phase of a
// sub-step; raised wave priority lets them issue whenever they are ready (the throughput-bound neighbour fills the rest):
// 0.832 -> 0.808 ms per discriminator sub-step, 0.574 -> 0.567 per generator sub-step.
#define XW_ODE_PRIO 3
__device__ __forceinline__ void xw_setprio(int p) {       // (s_setprio takes an immediate; p is uniform over the launch)
  if (p >= 3) __builtin_amdgcn_s_setprio(3);
  else if (p == 2) __builtin_amdgcn_s_setprio(2);
  else if (p == 1) __builtin_amdgcn_s_setprio(1);
}

// ---- stage activations kept from the forward pass ---------------------------------------------------------------------
// The sweeps need, for every stage of every step, the layer inputs relu(z_j), the tanh output and the stage input.
// Recomputing them from the checkpoint y_l costs the lone sweep wave 58 MFMAs and ~280 FP64 VALU instructions per step
// (two tanh blocks); HBM has 288 GB and is idle on this path, so the forward can simply store them:
//   act[l][tile of 16 paths][row][16],  l = 0 .. L-2,  rows: stage i -> i * M K + j K + k  (j < M-1: relu(z_j),
//   j = M-1: tanh(z_{M-1})), then the inputs of the stages i >= 1: S M K + (i-1) H + h.  Tile-major: what a wave stores
//   or loads for one step is ONE contiguous stretch (23 KB at 180 rows); path-major rows made it 180 pieces of 128 bytes,
//   32 KB apart, and the x-only sweep (183 MB in 0.1 ms) ran at the DRAM efficiency of that pattern.
//   Inside a tile every block of p <= 4 rows that one register of a chain tile covers is stored PATH-major,
//   [16 paths][p rows]: the partner wave of the duo sweep needs such a block as the B operand of a 4x4x4 MFMA -- lane
//   j + 4 b + 16 k = (row j, path 4 k + b) -- which is then lane-linear, 512 contiguous bytes.  Row-major, the four lanes of a
//   quad sat in four different 128-byte lines and the CU's address unit was stalled by the L1 a quarter of the launch
//   with three sweep tiles on a CU (TA_ADDR_STALLED_BY_TC 24.8 M -> 7.7 M cycles per three-job launch, average vector-memory
//   latency per instruction 29 -> 17 units; three concurrent jobs 170 -> 163 us, 16384 paths 244 -> 215 us, generator
//   sub-step 0.518 -> 0.510 ms).  What still separates two tiles of a CU (102 us alone, 148 us each) is the amount of
//   read data in flight per CU: 12.7 KB per field evaluation and tile at ~570 clocks of L2 latency.
// 180 doubles per path and step at (H, K, m) = (20, 10, 8), midpoint: 183 MB for 4096 paths x 32 times.
template <int H, int K, int M, int S> struct ActLayout {
  static constexpr int STAGE = M * K;
  static constexpr int YI = S * STAGE;
  static constexpr int ROWS = S * STAGE + (S - 1) * H;
  static constexpr int MASK = ROWS;                      // + 2 rows (64 words) per stage and mask word: the ReLU masks of SaveX
  static constexpr int MR = 2 * XW_MASK_WORDS(M);
  static constexpr int TOTAL = ROWS + MR * S;
};
// rows [row0, row0 + nrows) of the record <-> the first registers of a chain tile (row g + 4 r).  Addresses are
// formed as  (uniform row pointer) + (32-bit lane offset)  so that they cost SGPRs, not a VGPR pair per stored row.
struct ActLane {       // (unsigned: uniform pointer + zero-extended 32-bit lane offset is the scalar-base addressing form of the
                       //  global loads / stores -- with signed offsets every 4 KB of the record cost a 64-bit vector add)
  unsigned off;        // BYTES inside a full block of four rows: 8 (4 * column + g)
  unsigned off_part;   // inside the last, partially filled block of a K-row tile (p = K mod 4 rows): 8 (p * column + min(g, p - 1))
  unsigned off_part_st;   // the same for STORES: lanes without a row of their own (g >= p) get an offset beyond every record --
                          // the buffer's range check drops their store.  As a branch on the lane group (s_and_saveexec /
                          // s_cbranch_execz / s_or exec around one store per layer) the partial block cost the lone forward wave
                          // ~56 clocks per layer, 2.5 x the three stores themselves (tools/probe_store_cost.hip,
                          // profiles/r06_probe_store_cost.txt), and cut the time loop into a basic block per layer.
  bool valid;
};
#define XW_ACT_OOB 0x7fffff00u
__device__ __forceinline__ ActLane act_lane(int N, int col, bool valid, int krows) {
  const int g = xw_lane() >> 4, p = krows & 3;
  const int gp = p ? (g < p ? g : p - 1) : g;
  const unsigned part = 8u * (unsigned)((p ? p : 4) * col + gp);
  return ActLane{8u * (unsigned)(4 * col + g), part, (p == 0 || g < p) ? part : XW_ACT_OOB, valid};
}
// The forward pass writes the record through a BUFFER descriptor of the step's tile (base = the tile's 23 KB, built from
// scalars once per step): a store is then  descriptor + scalar row offset + 32-bit lane offset  and costs no vector
// instruction for its address.  With plain global stores the compiler folds all row offsets of a step onto one 64-bit
// vector address and re-bases it every 4 KB: 58 v_add_co / v_addc per step, each of which queues for the shared pipe.
typedef unsigned xw_u2v __attribute__((ext_vector_type(2)));
struct ActBuf {
  __amdgpu_buffer_rsrc_t rsrc;
};
__device__ __forceinline__ ActBuf act_buf(double* A, int bytes) {
  return ActBuf{__builtin_amdgcn_make_buffer_rsrc(A, 0, bytes, 0x00020000)};
}
__device__ __forceinline__ void act_store(const ActBuf& B, int row0, int nrows, int N, const ActLane& q, d4 v) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (4 * r < nrows) {
      const int so = (row0 + 4 * r) * N * 8;                                // uniform: the block of rows 4 r .. 4 r + 3
      // (the element goes through a scalar first: __builtin_bit_cast applied to v[r] directly reads element 0 of the vector)
      const double x = v[r];
      const xw_u2v w2 = {(unsigned)__double2loint(x), (unsigned)__double2hiint(x)};
      // (nt: streamed, read once, by a sweep; no branch: the lanes past a partial block's rows carry an out-of-range offset.
      //  Every caller's lanes are valid -- padding paths of the last tile hold finite copies and have slots of their own)
      __builtin_amdgcn_raw_buffer_store_b64(w2, B.rsrc, (int)(4 * r + 4 <= nrows ? q.off : q.off_part_st), so, 2);
    }
}
__device__ __forceinline__ d4 act_load(const double* __restrict__ A, int row0, int nrows, int N, const ActLane& q) {
  d4 v = xw_zero4();
  const char* base = reinterpret_cast<const char*>(A + (long)row0 * N);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (4 * r < nrows) {
      const char* __restrict__ blk = base + (long)(4 * r) * N * 8;         // uniform
      v[r] = __builtin_nontemporal_load(reinterpret_cast<const double*>(blk + (4 * r + 4 <= nrows ? q.off : q.off_part)));   // padding rows: any finite value
    }
  return v;
}

// streams the layer inputs of one stage into the activation store as they are produced (no register copy kept)
// FULL = false: only what a sweep WITHOUT weight gradients reads back (the tanh rows and the mask words)
template <int K, int M, bool FULL = true> struct SinkAct {
  const ActBuf& A;             // record of this step
  int row0, N;
  const ActLane& q;
  unsigned& bits;              // (z > 0) of the stage's pre-activations, pushed in (layer, register) order (SaveX)
  unsigned& bits_hi;           // (the second word: only where XW_MASK_WORDS(M) == 2)
  // relu of one pre-activation register: its bit (z > 0) goes into the mask word (v_cmp_gt_f64 + v_addc_co_u32), then
  // ONE v_max_f64 (3 vector instructions per register where compare, select, shift-or and two v_max_f64 were 4.5).  As a builtin the maximum comes with a canonicalising v_max_f64 z, z in front of it (45 extra vector
  // instructions per step); as inline assembly it would escape the hazard recogniser, which must keep a VALU read 6+ wait
  // states behind the MFMA that wrote z -- so the assembly takes the mask word as an (unused) operand: it then follows the
  // compare, a visible read of the same MFMA result for which the wait states have been inserted.
  __device__ __forceinline__ double relu(int, int kb, double z) const {
    const bool kb_last = kb == (K + 3) / 4 - 1;
    // (the compare is compiler-visible -- it is the read of z the hazard recogniser sees --, its lane mask goes into the
    //  assembly as a scalar pair and becomes the carry-in of  word = word + word + carry;  written in C the compiler
    //  turns the add-with-carry back into compare + select + shift-or)
    const unsigned long long open = __builtin_amdgcn_ballot_w64(z > 0.0);
    double r;
    // (a matrix instruction may not read the maximum in the two issue slots behind it -- without any wait state the x-only form,
    //  which stores nothing in between, fed stale registers to the next layer: round 6, test_ode_narrow_tile_sweeps -- and the
    //  compiler does not look into the assembly.  A layer's registers are rectified back to back and fence() keeps the next layer's
    //  matrix instructions behind all of them, so only the LAST register of a layer needs the two slots spelled out: the others
    //  have the next register's two instructions behind them.  A lone wave pays ~5 clocks per s_nop: 14 per time step now, 42 before.)
    if constexpr (XW_MASK_WORDS(M) == 2) {      // (the carry out of the low word shifts into the high one)
      if (kb_last) asm("v_addc_co_u32_e64 %1, vcc, %1, %1, %4\n\tv_addc_co_u32_e64 %2, vcc, %2, %2, vcc\n\tv_max_f64 %0, %3, 0\n\ts_nop 1" : "=v"(r), "+v"(bits), "+v"(bits_hi) : "v"(z), "s"(open) : "vcc");
      else asm("v_addc_co_u32_e64 %1, vcc, %1, %1, %4\n\tv_addc_co_u32_e64 %2, vcc, %2, %2, vcc\n\tv_max_f64 %0, %3, 0" : "=v"(r), "+v"(bits), "+v"(bits_hi) : "v"(z), "s"(open) : "vcc");
      return r;
    }
    if (kb_last) asm("v_addc_co_u32_e64 %1, vcc, %1, %1, %3\n\tv_max_f64 %0, %2, 0\n\ts_nop 1" : "=v"(r), "+v"(bits) : "v"(z), "s"(open) : "vcc");
    else asm("v_addc_co_u32_e64 %1, vcc, %1, %1, %3\n\tv_max_f64 %0, %2, 0" : "=v"(r), "+v"(bits) : "v"(z), "s"(open) : "vcc");
    return r;
  }
  __device__ __forceinline__ void fence() const { __builtin_amdgcn_sched_barrier(0); }
  __device__ __forceinline__ void z(int j, d4 r) const {
    if (FULL) act_store(A, row0 + j * K, K, N, q, r);
  }
  __device__ __forceinline__ void a(d4 v) const { act_store(A, row0 + (M - 1) * K, K, N, q, v); }
};

// store a chain-layout accumulator tile (rows r0.., cols c0..) into a row-major matrix
__device__ __forceinline__ void storeD(double* dst, int ld, int rows, int cols, int r0, int c0, d4 acc) {
  const int lane = xw_lane(), g = lane >> 4, c = c0 + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + g + 4 * r;
    if (row < rows && c < cols) dst[row * ld + c] = acc[r];
  }
}
// store column `col` of a chain-layout accumulator tile as a (strided) vector
__device__ __forceinline__ void storeDcol(double* dst, int stride, int rows, int r0, int col, d4 acc) {
  const int lane = xw_lane(), g = lane >> 4;
  if ((lane & 15) != col) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + g + 4 * r;
    if (row < rows) dst[(long)row * stride] = acc[r];
  }
}
// row sums over the 16 paths of a chain tile -> vector
__device__ __forceinline__ void storeRowSums(double* dst, int rows, int r0, d4 q) {
  const int lane = xw_lane(), g = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double s = xw_sum_over_n(q[r]);
    const int row = r0 + g + 4 * r;
    if ((lane & 15) == 0 && row < rows) dst[row] = s;
  }
}

// ---- end of a sweep: everything behind the time loop, for ONE tile of 16 paths in the chain layout ------------------------
// x-projection (cotangent of x, gradients of Win[:, :d] and Win.b), read-out layer gradients, the lift (initial layers):
// lam = cotangent of y_0, xpb = sum of the cotangents of z_0 over all field evaluations, ub0 = cotangent of u at the first
// time index, accFL / accFLb = sums of ubar y_l / ubar.  Shared by the 16-path sweeps (sweep_body) and by the narrow-tile
// sweep (xw_ode_n4.h), whose four waves hand these registers to their first wave through LDS.  lds: XW_SWEEP_TILES tiles.
template <int H, int K, bool PARAMS, bool ADJ, class StoreFieldGrads>
__device__ __forceinline__ void sweep_tail(const double* __restrict__ th, const UOff& o, int d, int N, int base, bool valid, int ncl,
                                           const double* __restrict__ xT, double sv, bool x_ones, const d4 (&lam)[Dim<H, K>::HT],
                                           d4 xpb, double ub0, const d4 (&accFL)[Dim<H, K>::HT], double accFLb,
                                           const d4 (&flw)[Dim<H, K>::HT], double* __restrict__ gx, double* __restrict__ gs,
                                           double* slab, double* lds, const StoreFieldGrads& store_field) {
  typedef Dim<H, K> D;
  const int lane = xw_lane(), g = lane >> 4, n = lane & 15;
  // ---- x-projection: cotangent of x, gradients of Win[:, :d] and Win.b -----------------------------------------
  if (gx != nullptr) {
    for (int rt = 0; rt < (d + 15) / 16; ++rt) {
      d4 v = xw_zero4();
      if (!ADJ) {                // (odeint_adjoint: x is not among the inputs the adjoint differentiates with respect to)
#pragma unroll
        for (int ks = 0; ks < D::KSK; ++ks) v = XW_MFMA(xw_fragAT(th + o.Win, o.ldin, K, d, 16 * rt, 4 * ks), xpb[ks], v);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * rt + g + 4 * r;
        if (i < d && valid) gx[(long)i * N + base + n] = v[r];
      }
    }
  }
  if (PARAMS) {
    xw_writeT(lds, xpb);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int ct = 0; ct < (d + 15) / 16; ++ct) {
      d4 acc = xw_zero4();
      const int i = 16 * ct + (lane & 15);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int pn = base + 4 * ks + (lane >> 4);
        const double b = (i < d && pn < N) ? xT[(long)i * N + pn] : 0.0;
        acc = XW_MFMA(xw_readT(lds, ks), b, acc);
      }
      storeD(slab + o.Win, o.ldin, K, d, 0, 16 * ct, acc);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    storeRowSums(slab + o.Winb, K, 0, xpb);
    store_field();                                         // (the field's own accumulators, where their owner keeps them)
#pragma unroll
    for (int ht = 0; ht < D::HT; ++ht) storeRowSums(slab + o.FLw, H, 16 * ht, accFL[ht]);
    const double sb = xw_sum_over_n(accFLb);
    if (lane == 0) slab[o.FLb] = sb;
  }

  // ---- initial layers: lam = cotangent of y_0 ----------------------------------------------------------------------
  {
    d4 a0[D::HT], a1[D::HT], y0[D::HT];
    lift<H, K>(th, o, sv, a0, a1, y0);
    d4 d1[D::HT], d0[D::HT];
    if (PARAMS) {
#pragma unroll
      for (int rt = 0; rt < D::HT; ++rt) {
#pragma unroll
        for (int ct = 0; ct < D::HT; ++ct) {
          d4 acc = xw_zero4();
          outer_acc(acc, lam[rt], a1[ct], lds);
          storeD(slab + o.IL4w, H, H, H, 16 * rt, 16 * ct, acc);
        }
        storeRowSums(slab + o.IL4b, H, 16 * rt, lam[rt]);
      }
    }
#pragma unroll
    for (int ht = 0; ht < D::HT; ++ht) {
      d4 v = xw_zero4();
#pragma unroll
      for (int ks = 0; ks < D::KSH; ++ks) v = XW_MFMA(xw_fragAT(th + o.IL4w, H, H, H, 16 * ht, 4 * ks), lam[ks >> 2][ks & 3], v);
#pragma unroll
      for (int r = 0; r < 4; ++r) d1[ht][r] = a1[ht][r] > 0.0 ? v[r] : 0.0;
    }
    if (PARAMS) {
#pragma unroll
      for (int rt = 0; rt < D::HT; ++rt) {
#pragma unroll
        for (int ct = 0; ct < D::HT; ++ct) {
          d4 acc = xw_zero4();
          outer_acc(acc, d1[rt], a0[ct], lds);
          storeD(slab + o.IL2w, H, H, H, 16 * rt, 16 * ct, acc);
        }
        storeRowSums(slab + o.IL2b, H, 16 * rt, d1[rt]);
      }
    }
    double gpart = 0.0;
#pragma unroll
    for (int ht = 0; ht < D::HT; ++ht) {
      d4 v = xw_zero4();
#pragma unroll
      for (int ks = 0; ks < D::KSH; ++ks) v = XW_MFMA(xw_fragAT(th + o.IL2w, H, H, H, 16 * ht, 4 * ks), d1[ks >> 2][ks & 3], v);
      const d4 w0 = xw_vecD(th + o.IL0w, H, 16 * ht);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        d0[ht][r] = a0[ht][r] > 0.0 ? v[r] : 0.0;
        gpart += w0[r] * d0[ht][r];
      }
      if (PARAMS) {
        storeRowSums(slab + o.IL0w, H, 16 * ht, d0[ht] * sv);
        storeRowSums(slab + o.IL0b, H, 16 * ht, d0[ht]);
      }
    }
    double gsn = xw_sum_over_g(gpart);
    if (PARAMS && gs != nullptr && x_ones) {
      // The x outputs of this launch stand for the helper backward u.backward(ones) (src/loss.py:55) while the
      // parameter gradients use ubar, which differs from ones at the first time index only (the initial-value penalty).
      // gx never sees that entry (no step is reversed after it), d/d start does, linearly through the lift:
      // subtract the lift's response to flw * (ubar_0 - 1).
      const double dub = ub0 - (valid ? 1.0 : 0.0);
      d4 e1[D::HT];
#pragma unroll
      for (int ht = 0; ht < D::HT; ++ht) {
        d4 v = xw_zero4();
#pragma unroll
        for (int ks = 0; ks < D::KSH; ++ks) v = XW_MFMA(xw_fragAT(th + o.IL4w, H, H, H, 16 * ht, 4 * ks), flw[ks >> 2][ks & 3], v);
#pragma unroll
        for (int r = 0; r < 4; ++r) e1[ht][r] = a1[ht][r] > 0.0 ? v[r] : 0.0;
      }
      double cpart = 0.0;
#pragma unroll
      for (int ht = 0; ht < D::HT; ++ht) {
        d4 v = xw_zero4();
#pragma unroll
        for (int ks = 0; ks < D::KSH; ++ks) v = XW_MFMA(xw_fragAT(th + o.IL2w, H, H, H, 16 * ht, 4 * ks), e1[ks >> 2][ks & 3], v);
        const d4 w0 = xw_vecD(th + o.IL0w, H, 16 * ht);
#pragma unroll
        for (int r = 0; r < 4; ++r) cpart += a0[ht][r] > 0.0 ? w0[r] * v[r] : 0.0;
      }
      gsn -= dub * xw_sum_over_g(cpart);
    }
    if (gs != nullptr && g == 0 && valid) gs[base + n] = gsn;
  }
}

// ---- kernel tables (host) ----------------------------------------------------------------------------------------------------------
// Every stepper kernel has one signature per direction.  A table holds the kernels of one direction in this object,
// [depth - 1].k[slot] (the slots: xw_ode_select.h); AT<M, SLOT>::k is the one place that names the instantiation, and the order
// of the slots is the order of the kernels in the code object.  Depths the object does not hold (XW_ODE_ONLY_M) are rows of null
// pointers: the entry points answer XW_E_DIMS (depth_compiled).
template <class Jobs> using OdeKernel = void (*)(const Jobs, const double*, const double*, int, int);
template <class Jobs, int SLOTS> struct KernelRow { OdeKernel<Jobs> k[SLOTS]; };
template <template <int, int> class AT, class Jobs, int M, int... SLOT>
constexpr KernelRow<Jobs, sizeof...(SLOT)> kernel_row(std::integer_sequence<int, SLOT...>) {
  if constexpr (XW_ODE_HAS_DEPTH(M)) return {{AT<M, SLOT>::k...}};
  else return {};
}
template <template <int, int> class AT, class Jobs, int SLOTS, int... M0>
constexpr std::array<KernelRow<Jobs, SLOTS>, sizeof...(M0)> kernel_rows(std::integer_sequence<int, M0...>) {
  return {{kernel_row<AT, Jobs, M0 + 1>(std::make_integer_sequence<int, SLOTS>{})...}};
}
template <template <int, int> class AT, class Jobs, int SLOTS> constexpr auto kernel_table() {
  return kernel_rows<AT, Jobs, SLOTS>(std::make_integer_sequence<int, XW_ODE_DEPTHS>{});
}
}  // namespace
