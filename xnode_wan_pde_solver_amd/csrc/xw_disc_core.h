// xw_disc_core.h -- what the three sources of the adversarial test network v_phi share (xw_disc_fwd.hip, xw_disc_rec.hip,
// xw_disc_bwd.hip): the tile geometry of a width, the point locator, the input layer, the compiled widths and the slab count.
//
// Replaces discriminator.forward (src/model.py:37-47 of the reference), the helper backward that produces
// nabla phi (src/loss.py:60-63) and the autograd replay that produces phi's gradient (src/training.py:161).
//
// v_phi is a W-wide (50) MLP with ONE weight-tied hidden layer applied q (9) times: a real dense contraction
// [W x W] x [W x points] -- the only part of the hot path where the hidden width makes MFMA tiles pay
// (4 row tiles x 13 k-steps of v_mfma_f64_16x16x4_f64 per layer per 16 points, 75 % useful after padding 50 -> 64/52).
//
//   k_disc_fwd : value and d/dt (forward-mode tangent: the weak form needs d(phi)/dt at every sample point but
//   (xw_disc_fwd.hip)  nabla_x phi only at the initial time).  Vh rows 0..47 as 39 A-fragments in LDS
//                (shared by the 4 waves of a block, two waves per SIMD), rows 48, 49 on the vector ALU; activations never
//                leave the chain layout.  HBM traffic: x, t in, v, dv/dt out -- plus, on request, the record of layer
//                inputs (500 doubles per point) that k_disc_rec reads instead of recomputing the forward.
//   k_disc_rec : parameter gradient from that record: reverse chain + MFMA outer products (48 x 48 core on 16x16x4 tiles, the
//   (xw_disc_rec.hip)  two edges of the 50 x 51 matrix on 4x4x4 blocks), 78 KB of LDS, two blocks/CU.
//   k_disc_bwd : recomputes the forward for a tile of 16 points per wave (activations stay in registers), runs the
//   (xw_disc_bwd.hip)  reverse chain with Vh^T fragments from LDS, and accumulates  dVh += delta_{j+1} (x) relu(a_j)  as MFMA
//                outer products over the points (LDS transpose; 4 waves of a block own one 16-row band of dVh each).
//                Optionally also returns the input gradient (nabla_x v, dv/dt) -- used for nabla phi at t0.
//
// All instantiations of one kernel template stay in ONE source: what else a translation unit holds moves the compiler's choices
// (profiles/r23_testnet_split.md), and tests/test_testnet_inventory_host.py pins it.
#pragma once
#include "xw_common.h"
#include "xw_generic.h"

// (internal linkage, like the kernels that use these: every source gets its own copy and nothing of it is a symbol)
namespace {

template <int W> struct VDim {
  static constexpr int MT = (W + 15) / 16;
  static constexpr int KS = (W + 3) / 4;
  // rows of the last (partial) row tile.  A 16-row MFMA tile for 2 live rows (W = 50) is 13 x 2 wasted 64-cycle matrix
  // instructions per layer: when the tail is short the forward kernel contracts those rows on the vector ALU instead.
  static constexpr int TR = W - 16 * (MT - 1);
  static constexpr bool VTAIL = TR <= 3;
  static constexpr int MTF = VTAIL ? MT - 1 : MT;     // row tiles that go through the matrix pipe in k_disc_fwd
  // live registers (4-row groups) of row tile mt, counting the ones row W of the outer products: elementwise work,
  // checkpoints and transposes skip the padding rows (a lone wave pays ~9 clocks per FP64 VALU instruction)
  __device__ static constexpr int LR(int mt) { return (W + 1 - 16 * mt) >= 16 ? 4 : (W + 1 - 16 * mt + 3) / 4; }
  // W not a multiple of 16: a padding row of the last tile is set to one, so that column W of the dVh outer products
  // collects dVh.b for free; otherwise (W = 64) the bias gradient is summed on the vector ALU
  static constexpr bool BIASROW = (W % 16) != 0;
  // (MT = 4: widths 50 and 64, every kernel of the family; MT = 6, 8: the 96- and 128-wide containers -- forward and reverse from the record)
  static_assert(MT == 4 || MT == 6 || MT == 8, "row tiles of the compiled widths");
};

// point -> (time, path) ; path mode: p = l*N + n ; point mode (tpp != null): p = n, L == 1
struct Pt {
  int p, n;
  bool valid;
  double t;
};
__device__ __forceinline__ Pt locate(long tile, long P, int N, const double* __restrict__ tf, const double* __restrict__ tpp) {
  Pt q;
  const long p = tile * 16 + (xw_lane() & 15);
  q.valid = p < P;
  const long pc = q.valid ? p : P - 1;
  q.p = (int)pc;
  if (tpp != nullptr) {
    q.n = (int)pc;
    q.t = tpp[pc];
  } else {
    const int l = (int)(pc / N);
    q.n = (int)(pc - (long)l * N);
    q.t = tf[l];
  }
  return q;
}

// input layer a0 = Vin [t; x] + b  (and its t-tangent = Vin[:, 0])
template <int W>
__device__ __forceinline__ void input_layer(const double* __restrict__ ph, const VOff& o, const double* __restrict__ xT,
                                            int N, int d, const Pt& q, d4 (&a)[VDim<W>::MT], d4 (&ad)[VDim<W>::MT]) {
  typedef VDim<W> D;
  const int g = xw_lane() >> 4;
#pragma unroll
  for (int mt = 0; mt < D::MT; ++mt) {
    ad[mt] = xw_vecD_strided(ph + o.Vin, o.ldin, W, 16 * mt);
    a[mt] = xw_vecD(ph + o.Vinb, W, 16 * mt) + ad[mt] * q.t;
  }
  for (int ks = 0; ks < (d + 3) / 4; ++ks) {
    const int i = 4 * ks + g;
    const double b = i < d ? xT[(long)i * N + q.n] : 0.0;
#pragma unroll
    for (int mt = 0; mt < D::MT; ++mt) a[mt] = XW_MFMA(xw_fragA(ph + o.Vin + 1, o.ldin, W, d, 16 * mt, 4 * ks), b, a[mt]);
  }
}

#define XW_QMAX 16   // deepest test network whose ReLU masks fit the LDS stash of k_disc_fwd's fused input gradient

// compiled widths: 50 (the reference's YAML; all kernels) and 64 (container of the widths above 50: forward with the
// fused input gradient + reverse from the record, any depth; no recomputing reverse kernels)
inline bool disc_width_ok(int W) { return W == 50 || W == 64 || W == 96 || W == 128; }
// (other widths up to 128: the generic path of xw_generic.hip, always from a record -- row-major there, [rows][columns])

// slabs of a parameter gradient over P points, one per block of the reverse kernels (k_disc_rec, k_disc_bwd, k_dt_bwd of
// xw_disc_tiled.hip and the generic kg_disc_bwd): 64 points per block up to two resident blocks per CU, grid-stride beyond
inline int bwd_blocks(long P) {
  long nsuper = (P + 63) / 64;
  return (int)(nsuper < 512 ? nsuper : 512);
}

}  // namespace

// k_disc_rec<W, 0, ng, tsum> of xw_disc_rec.hip on `blocks` blocks (one slab each); XW_E_DIMS for a key that is not compiled.
// Called by xw_disc_bwd (xw_disc_bwd.hip), which has checked the arguments and chosen the key.
XWG_HIDDEN int xw_disc_rec_launch(int W, int ng, bool tsum, int blocks, const double* xT, const double* t, const double* tpp,
                                  const double* phi, const double* vbar, int N, int L, int d, double* gslab, const double* act,
                                  int q, void* stream);
