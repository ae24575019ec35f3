// xw_ode_mfma4.h -- the stepper's field on v_mfma_f64_4x4x4: the form of the narrow containers (20, 10) and (32, 12), i.e. of
// every build of xw_ode_fwd.h / xw_ode.hip WITHOUT -DXW_ODE_WIDE16.  Included once: the field (operands, evaluation, vector-
// Jacobian product, gradient accumulators, the duo sweep's LDS plan), then storing the gradients and the duo sweep's second wave.
#pragma once
#include "xw_ode_core.h"

namespace {

static_assert(XW_ODE_K <= 15, "row K of the 16-row K-tile is the ones row that collects the bias gradients");
static_assert(Dim<XW_ODE_H, XW_ODE_K>::HT <= 2 && Dim<XW_ODE_H, XW_ODE_K>::CT <= 3, "H <= 32");
// The field's layers run on v_mfma_f64_4x4x4_4b_f64: one instruction = a 4x4 weight block times 4 rows x 16 paths of
// the chain layout (its four "blocks" are the four groups of 4 paths; the weight block is replicated over them -- the
// CBSZ/ABID broadcast does nothing on the f64 form, profiles/r02_probe_mfma4b.txt).  A [K x K] layer is KB x KB = 9
// instructions of 18 clocks on KB INDEPENDENT accumulators instead of 3 dependent 16x16x4 instructions of 64 + 17 clocks
// on a tile with 10 of 16 rows live: 185 instead of 276 clocks per layer for the lone wave of a stepper tile, 16 % less
// matrix-pipe time when the chip is shared (same probe).
template <int H, int K> struct FieldW {      // forward operands: 4x4 blocks (row block, k block)
  double Wy[Dim<H, K>::KB][Dim<H, K>::HB];   // Win[:, d+1:]  [K x H]
  double Wh[Dim<H, K>::KB][Dim<H, K>::KB];   // Wh            [K x K]
  double Wo[Dim<H, K>::HB][Dim<H, K>::KB];   // Wo            [H x K]
  d4 wt, bh;                                 // Win[:, d] (time column), Wh.b
  d4 bo[Dim<H, K>::HT];                      // Wo.b
};
template <int H, int K> struct FieldWT {     // transposed operands for the vector-Jacobian product
  double WyT[Dim<H, K>::HB][Dim<H, K>::KB];  // [H x K]
  double WhT[Dim<H, K>::KB][Dim<H, K>::KB];  // [K x K]
  double WoT[Dim<H, K>::KB][Dim<H, K>::HB];  // [K x H]
};
template <int H, int K>
__device__ __forceinline__ void load_field(const double* __restrict__ th, const UOff& o, int d, FieldW<H, K>& w) {
  typedef Dim<H, K> D;
  const double* Wy = th + o.Win + d + 1;
#pragma unroll
  for (int rb = 0; rb < D::KB; ++rb) {
#pragma unroll
    for (int kb = 0; kb < D::HB; ++kb) w.Wy[rb][kb] = xw_fragA4(Wy, o.ldin, K, H, 4 * rb, 4 * kb);
#pragma unroll
    for (int kb = 0; kb < D::KB; ++kb) w.Wh[rb][kb] = xw_fragA4(th + o.Wh, K, K, K, 4 * rb, 4 * kb);
  }
#pragma unroll
  for (int rb = 0; rb < D::HB; ++rb)
#pragma unroll
    for (int kb = 0; kb < D::KB; ++kb) w.Wo[rb][kb] = xw_fragA4(th + o.Wo, K, H, K, 4 * rb, 4 * kb);
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) w.bo[ht] = xw_vecD(th + o.Wob, H, 16 * ht);
  w.wt = xw_vecD_strided(th + o.Win + d, o.ldin, K, 0);
  w.bh = xw_vecD(th + o.Whb, K, 0);
}
template <int H, int K>
__device__ __forceinline__ void load_field_T(const double* __restrict__ th, const UOff& o, int d, FieldWT<H, K>& w) {
  typedef Dim<H, K> D;
  const double* Wy = th + o.Win + d + 1;
#pragma unroll
  for (int rb = 0; rb < D::HB; ++rb)
#pragma unroll
    for (int kb = 0; kb < D::KB; ++kb) w.WyT[rb][kb] = xw_fragAT4(Wy, o.ldin, K, H, 4 * rb, 4 * kb);
#pragma unroll
  for (int rb = 0; rb < D::KB; ++rb) {
#pragma unroll
    for (int kb = 0; kb < D::KB; ++kb) w.WhT[rb][kb] = xw_fragAT4(th + o.Wh, K, K, K, 4 * rb, 4 * kb);
#pragma unroll
    for (int kb = 0; kb < D::HB; ++kb) w.WoT[rb][kb] = xw_fragAT4(th + o.Wo, K, H, K, 4 * rb, 4 * kb);
  }
}
template <int H, int K, int M, bool OUT = true, class Sink>
__device__ __forceinline__ void field_fwd(const FieldW<H, K>& w, double t, d4 xp, const d4 (&y)[Dim<H, K>::HT],
                                          d4 (&out)[Dim<H, K>::HT], const Sink& sink) {
  typedef Dim<H, K> D;
  // (k block outer, row block inner: consecutive instructions write different accumulators)
  d4 z = xw_zero4();
#pragma unroll
  for (int r = 0; r < D::KB; ++r) z[r] = fma(w.wt[r], t, xp[r]);
#pragma unroll
  for (int kb = 0; kb < D::HB; ++kb)
#pragma unroll
    for (int rb = 0; rb < D::KB; ++rb) z[rb] = XW_MFMA4(w.Wy[rb][kb], y[kb >> 2][kb & 3], z[rb]);
#pragma unroll
  for (int j = 0; j < M - 1; ++j) {
    d4 r = xw_zero4();
#pragma unroll
    for (int kb = 0; kb < D::KB; ++kb) r[kb] = sink.relu(j, kb, z[kb]);
    sink.fence();
    sink.z(j, r);
    d4 nz = w.bh;
#pragma unroll
    for (int kb = 0; kb < D::KB; ++kb)
#pragma unroll
      for (int rb = 0; rb < D::KB; ++rb) nz[rb] = XW_MFMA4(w.Wh[rb][kb], r[kb], nz[rb]);
    z = nz;
  }
  d4 a = xw_zero4();
#pragma unroll
  for (int kb = 0; kb < D::KB; ++kb) a[kb] = xw_tanh(z[kb]);
  sink.a(a);
  if (!OUT) return;
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) out[ht] = w.bo[ht];
#pragma unroll
  for (int kb = 0; kb < D::KB; ++kb)
#pragma unroll
    for (int rb = 0; rb < D::HB; ++rb) out[rb >> 2][rb & 3] = XW_MFMA4(w.Wo[rb][kb], a[kb], out[rb >> 2][rb & 3]);
}

// parameter-gradient accumulators of the field (chain-layout tiles of the gradient matrices)
template <int H, int K> struct FieldG {
  d4 Wh;                                          // rows K, cols K (+ column K = bias via a ones row)
  d4 Wy[Dim<H, K>::CT];                           // rows K, cols H (+ column H = time column)
  d4 Wo[Dim<H, K>::HT];                           // rows H, cols K (+ column K = bias)
};
template <int H, int K, int M> struct DuoPlan {
  static constexpr int HT = Dim<H, K>::HT;
  static constexpr int NQ = HT + (M - 1) + 1;     // Q tiles of one field evaluation: cot(out) x HT, cot(z_{j+1}) for j = M-2 .. 0, cot(z_0)
  // Tiles are packed by their LIVE rows (4-row groups): a partner reads 16 rows of every tile (xw_readT), the rows past a
  // tile's own are its successor's -- finite values that only reach accumulator rows which are never stored.  43 -> 16 KB
  // per buffer at (20, 10, 8): 4 instead of 2 resident sweep blocks per CU (the third job of a sub-step queued for LDS).
  static constexpr int HLAST = 4 * Dim<H, K>::HR(HT - 1);                   // rows of the last cot(out) tile
  static constexpr int KROWS = 4 * Dim<H, K>::KSK;                          // rows of a K-tile
  __device__ static constexpr int off(int t) {                             // first double of tile t
    return XW_TSTRIDE * (t < HT ? 16 * t : 16 * (HT - 1) + HLAST + KROWS * (t - HT));
  }
  static constexpr int BUF = XW_TSTRIDE * (16 * (HT - 1) + HLAST + KROWS * M + 16);   // (+ 16 rows: reads past the last tile)
  static_assert(BUF >= 3 * XW_TTILE, "the chain wave's epilogue borrows a buffer for its three transpose tiles");
};
// vector-Jacobian product of one field evaluation.  ob: cotangent of F's output; returns the cotangent of the y input
// in yb, adds the cotangent of z0 into xpb (= cotangent of the x-projection and of Win.b), and (PARAMS) accumulates the
// parameter gradients (outer products over the 16 paths; in the 4x4x4 form a row of ones / the time row in the R tile makes the bias and
// time-column gradients ride along as an extra accumulator column).
// OUTER: 0 = no weight gradients, 1 = this wave forms them itself (outer products through its own LDS tiles),
//        2 = "duo" sweep: this wave only posts the cotangent tiles (transposed) into `lds` = the evaluation's Q buffer
//            (DuoPlan), a partner wave of the block contracts them with the activations it loads itself.
template <int H, int K, int M, int OUTER, class SV>
__device__ __forceinline__ void field_vjp(const FieldW<H, K>& w, const FieldWT<H, K>& wT, double t, const SV& sv,
                                          const d4 (&yin)[Dim<H, K>::HT], const d4 (&ob)[Dim<H, K>::HT],
                                          d4 (&yb)[Dim<H, K>::HT], d4& xpb, FieldG<H, K>& G, double* lds) {
  typedef Dim<H, K> D;
  constexpr bool PARAMS = OUTER == 1;
  static_assert(D::HT <= 2, "two Q / R tile pairs in the LDS plan");
  const double* rt1 = lds + 2 * XW_TTILE;
  OuterOps o0;
  double q1[4];
  if (OUTER == 2) {
#pragma unroll
    for (int ht = 0; ht < D::HT; ++ht) {
      if (ht == 0) xw_writeT_pn<D::HR(0)>(lds, ob[0]);
      else xw_writeT_pn<D::HR(D::HT - 1)>(lds + DuoPlan<H, K, M>::off(ht), ob[ht]);
    }
  }
  if (PARAMS) {
    outer_post_ones<D::HR(0), K>(ob[0], sv.a, lds);
    if (D::HT > 1) {
      xw_writeT_n<D::HR(D::HT - 1)>(lds + 3 * XW_TTILE, ob[D::HT - 1]);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    outer_fetch(o0, lds, rt1);
    if (D::HT > 1) outer_fetch1(q1, lds + 3 * XW_TTILE);
  }
  d4 ab = xw_zero4();
#pragma unroll
  for (int kb = 0; kb < D::HB; ++kb)
#pragma unroll
    for (int rb = 0; rb < D::KB; ++rb) ab[rb] = XW_MFMA4(wT.WoT[rb][kb], ob[kb >> 2][kb & 3], ab[rb]);
  if (PARAMS) {
    outer_fire(G.Wo[0], o0.a, o0.b);
    if (D::HT > 1) outer_fire(G.Wo[D::HT - 1], q1, o0.b);
  }
  d4 zb = xw_zero4();
#pragma unroll
  for (int r = 0; r < D::KSK; ++r) zb[r] = ab[r] * (1.0 - sv.a[r] * sv.a[r]);
#pragma unroll
  for (int j = M - 2; j >= 0; --j) {
    if constexpr (PARAMS) {
      outer_post_ones<D::KSK, K>(zb, sv.z[j], lds);
      outer_fetch(o0, lds, rt1);
    }
    if (OUTER == 2) xw_writeT_pn<D::KSK>(lds + DuoPlan<H, K, M>::off(D::HT + (M - 2 - j)), zb);
    d4 tt = xw_zero4();
#pragma unroll
    for (int kb = 0; kb < D::KB; ++kb)
#pragma unroll
      for (int rb = 0; rb < D::KB; ++rb) tt[rb] = XW_MFMA4(wT.WhT[rb][kb], zb[kb], tt[rb]);
    if (PARAMS) outer_fire(G.Wh, o0.a, o0.b);
#pragma unroll
    for (int r = 0; r < D::KSK; ++r) zb[r] = sv.gate(j, r, tt[r]);
  }
#pragma unroll
  for (int r = 0; r < D::KSK; ++r) xpb[r] += zb[r];
  if (OUTER == 2) xw_writeT_pn<D::KSK>(lds + DuoPlan<H, K, M>::off(D::HT + M - 1), zb);
  double rr[D::CT][4];
  if (PARAMS) {
    // one Q tile (the cotangent of z0) against the column tiles of [y ; t]: the time row makes column H collect the
    // time-column gradient (row H & 15 of tile H >> 4: a tile of its own when H is a multiple of 16)
    xw_writeT_n<D::KSK>(lds, zb);
#pragma unroll
    for (int ct = 0; ct < D::CT; ++ct) {
      d4 yy = ct < D::HT ? yin[ct < D::HT ? ct : 0] : xw_zero4();
      if (ct == (H >> 4)) set_row(yy, H & 15, t);
      double* rt = lds + (ct == 0 ? 1 : 3 + ct) * XW_TTILE;            // tiles 1, 4, 5
      if (ct == 0) xw_writeT_n<D::HR1(0)>(rt, yy);
      else if (ct == 1) xw_writeT_n<D::HR1(1)>(rt, yy);
      else xw_writeT_n<D::HR1(2)>(rt, yy);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_sched_barrier(0);
    outer_fetch1(o0.a, lds);
#pragma unroll
    for (int ct = 0; ct < D::CT; ++ct) outer_fetch1(rr[ct], lds + (ct == 0 ? 1 : 3 + ct) * XW_TTILE);
  }
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) yb[ht] = xw_zero4();
#pragma unroll
  for (int kb = 0; kb < D::KB; ++kb)
#pragma unroll
    for (int rb = 0; rb < D::HB; ++rb) yb[rb >> 2][rb & 3] = XW_MFMA4(wT.WyT[rb][kb], zb[kb], yb[rb >> 2][rb & 3]);
  if (PARAMS) {
#pragma unroll
    for (int ct = 0; ct < D::CT; ++ct) outer_fire(G.Wy[ct], o0.a, rr[ct]);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- the field gradients: into the slab; the duo sweep's second wave
// the field's weight-gradient accumulators -> one slab
template <int H, int K, bool HID = true, bool IO = true>
__device__ __forceinline__ void store_field_grads(double* slab, const UOff& o, int d, const FieldG<H, K>& G) {
  typedef Dim<H, K> D;
  if (HID) {
    storeD(slab + o.Wh, K, K, K, 0, 0, G.Wh);
    storeDcol(slab + o.Whb, 1, K, 0, K, G.Wh);
  }
  if (!IO) return;
#pragma unroll
  for (int ct = 0; ct < (H + 1 + 15) / 16; ++ct) {
    storeD(slab + o.Win + d + 1, o.ldin, K, H, 0, 16 * ct, G.Wy[ct]);
    if (ct == (H >> 4)) storeDcol(slab + o.Win + d, o.ldin, K, 0, H & 15, G.Wy[ct]);
  }
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) {
    storeD(slab + o.Wo, K, H, K, 16 * ht, 0, G.Wo[ht]);
    storeDcol(slab + o.Wob, 1, H, 16 * ht, K, G.Wo[ht]);
  }
}
// ---- the duo sweep's second wave: weight gradients of the field -------------------------------------------------------
// For every field evaluation (same order as the chain wave, one evaluation behind it):
//     dWo += cot(out) (x) [tanh(z_{m-1}) ; 1]     dWh += sum_j cot(z_{j+1}) (x) [relu(z_j) ; 1]     dWy += cot(z_0) (x) [y_in ; t]
// contractions over the 16 paths of the tile, on v_mfma_f64_4x4x4_4b_f64 with the instruction's four blocks = the four
// GROUPS OF FOUR PATHS:  acc[g][i][j] += sum_{k<4} q[4 rb + i][path 4 g + k] * r[4 cb + j][path 4 g + k].  One instruction
// covers a 4 x 4 block of the gradient over ALL 16 paths (every block does useful work, 4-row / 4-column granularity: dWh
// is 3 x 3 instructions per layer, 76 % of their multiply-adds useful, against 4 16x16x4 instructions at 43 %: 96 x 18
// instead of 44 x 66 clocks per evaluation); the four per-group partial sums of an accumulator are added ONCE, at the end
// of the sweep.  A operands: the cotangent tiles the chain wave posted (transposed) in LDS, lane (i, g, k) reads row
// 4 rb + i, path 4 g + k.  B operands: the layer inputs straight from the activation store / the checkpoints in that same
// lane layout, fetched a whole evaluation ahead (a register is reloaded for the next evaluation right behind the last
// instruction that reads it).  Rows a block has no data for (the ones row that collects the bias gradient, zero padding)
// read a constant table -- every lane loads, the loop stays ONE basic block (see duo_b_ptr).
typedef const double __attribute__((address_space(1)))* xw_gptr;
__device__ const double xw_duo_const[2][16] = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
                                               {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}};
// where the operands of field evaluation e (chain-wave order: steps L-2 .. 0, stages S-1 .. 0) come from
template <int H, int K, int M, int METHOD> struct DuoSrc {
  const double* __restrict__ A;      // activation record of the step
  const double* __restrict__ Yl;     // checkpoint y_l of the step (stage 0's input)
  int i;                             // stage
  double ti;                         // its time
  __device__ __forceinline__ DuoSrc(const double* __restrict__ Y, const double* __restrict__ act,
                                    const double* __restrict__ tf, int e, int L, int N, int tile) {
    typedef RK<METHOD> T;
    typedef ActLayout<H, K, M, T::S> AL;
    const int l = L - 2 - e / T::S;
    i = T::S - 1 - e % T::S;
    A = act + ((long)l * ((N + 15) >> 4) + tile) * (AL::TOTAL * 16);
    Yl = Y + (long)l * H * N;
    const double t0 = tf[l];
    ti = t0 + T::c(i) * (tf[l + 1] - t0);
  }
};
template <int H, int K, int M> struct Duo4 {
  static constexpr int KB1 = (K + 1 + 3) / 4;     // column blocks of [layer input ; 1]
  static constexpr int HB1 = (H + 1 + 3) / 4;     // column blocks of [y ; t]
  static constexpr int KB = Dim<H, K>::KB, HB = Dim<H, K>::HB;
};
// B operand of column block cb of a K-row activation tile [rows ; ones row ; zero padding]
// (explicitly GLOBAL pointers: a select between a kernel argument and the address of a __device__ object is a generic
//  pointer to the compiler, and flat loads return out of order -- every use would drain vmcnt(0))
template <int H, int K, int M, int METHOD>
__device__ __forceinline__ double duo_load_act(const DuoSrc<H, K, M, METHOD>& s, int jrow /* layer, M-1 = tanh */, int cb) {
  typedef ActLayout<H, K, M, RK<METHOD>::S> AL;
  const int lane = xw_lane(), j = lane & 3;
  const int row = 4 * cb + j;
  // lane j + 4 b + 16 k = (row 4 cb + j, path 4 k + b): lane-linear inside a full path-major block; a partial last block
  // of p rows holds (row, path) at p * path + row
  const int p = K - 4 * cb < 4 ? K - 4 * cb : 4;               // (compile-time after unrolling)
  const int off = p == 4 ? lane : p * (lane >> 2) + j;
  const xw_gptr src = row < K ? (xw_gptr)(s.A + (s.i * AL::STAGE + jrow * K + 4 * cb) * 16 + off) : (xw_gptr)&xw_duo_const[row == K ? 1 : 0][0];
  return __builtin_nontemporal_load(src);
}
// ... of [y_in ; t ; zero padding]: rows of y_l (checkpoints, stage 0) or of the activation record (later stages);
// branch-free (the loop must stay one basic block, or the compiler's wait-count bookkeeping falls back to vmcnt(0) at
// its head); the time row is patched in where the block is USED (a select here would wait for the load)
template <int H, int K, int M, int METHOD>
__device__ __forceinline__ double duo_load_y(const DuoSrc<H, K, M, METHOD>& s, int cb, int N, int tile) {
  typedef ActLayout<H, K, M, RK<METHOD>::S> AL;
  static_assert(H % 4 == 0, "the stage inputs are whole path-major blocks");
  const int lane = xw_lane(), j = lane & 3, b = (lane >> 2) & 3, k = lane >> 4;
  const int row = 4 * cb + j;
  const bool first = s.i == 0;                                // (wave-uniform)
  // stage 0: the checkpoint y_l [H][N] (row-major); later stages: path-major blocks of the record, lane-linear
  const long col = (long)tile * 16 + 4 * k + b;
  const double* __restrict__ src_y = s.Yl + (long)row * N + (col < N - 1 ? col : N - 1);
  const double* __restrict__ src_a = s.A + (long)(AL::YI + (s.i > 0 ? s.i - 1 : 0) * H + 4 * cb) * 16 + lane;
  const xw_gptr src = row < H ? (xw_gptr)(first ? src_y : src_a) : (xw_gptr)&xw_duo_const[0][0];
  return __builtin_nontemporal_load(src);
}
// A operand: rows 4 rb .. 4 rb + 3 of a transposed cotangent tile in LDS, posted by xw_writeT_pn (tile[row * XW_TSTRIDE +
// 4 (path & 3) + (path >> 2)]): lane i + 4 b + 16 k = (row i, path 4 k + b) sits at position 4 b + k
__device__ __forceinline__ double duo_readA(const double* tile, int rb) {
  const int l = xw_lane();
  return tile[(4 * rb + (l & 3)) * XW_TSTRIDE + ((l >> 2) & 3) * 4 + (l >> 4)];
}
// sum of an accumulator's four path-group partials (lane bits 2, 3), then element (row 4 rb + i, col 4 cb + j) from lane j + 16 i
__device__ __forceinline__ double duo_fold(double x) {
  x += __shfl_xor(x, 4);
  x += __shfl_xor(x, 8);
  return x;
}
template <int H, int K, int M, int METHOD>
__device__ __forceinline__ void duo_outer(const BwdJobs& jobs, const double* __restrict__ tf, const double* __restrict__ th,
                                          int L, int d, const double* qbuf, int vb) {
  typedef Dim<H, K> D;
  typedef RK<METHOD> T;
  typedef DuoPlan<H, K, M> P;
  typedef Duo4<H, K, M> Q;
  typedef DuoSrc<H, K, M, METHOD> Src;
  constexpr int NH = M > 1 ? M - 1 : 1;
  xw_setprio(jobs.prio);          // (a lower priority for this wave than for the chain: no difference)
  const int job = find_job(jobs, vb);
  const double* __restrict__ Y = jobs.Y[job];
  const double* __restrict__ act = jobs.act[job];
  const int N = jobs.N[job];
  const int tile = vb - jobs.tile0[job];
  const int lane = xw_lane();
  const UOff o = u_offsets(d, H, K);
  double gWh[Q::KB][Q::KB1], gWo[Q::HB][Q::KB1], gWy[Q::KB][Q::HB1];
#pragma unroll
  for (int rb = 0; rb < Q::KB; ++rb) {
#pragma unroll
    for (int cb = 0; cb < Q::KB1; ++cb) gWh[rb][cb] = 0.0;
#pragma unroll
    for (int cb = 0; cb < Q::HB1; ++cb) gWy[rb][cb] = 0.0;
  }
#pragma unroll
  for (int rb = 0; rb < Q::HB; ++rb)
#pragma unroll
    for (int cb = 0; cb < Q::KB1; ++cb) gWo[rb][cb] = 0.0;
  double Ra[Q::KB1], Rr[NH][Q::KB1], Ry[Q::HB1];          // B operands of the evaluation in flight
  const int E = (L - 1) * T::S;                            // field evaluations of the sweep
  double ti_cur = 0.0;                                     // time of the evaluation whose operands are in R*
  if (E > 0) {
    const Src s0(Y, act, tf, 0, L, N, tile);
    ti_cur = s0.ti;
#pragma unroll
    for (int cb = 0; cb < Q::KB1; ++cb) Ra[cb] = duo_load_act<H, K, M, METHOD>(s0, M - 1, cb);
#pragma unroll
    for (int jj = M - 2; jj >= 0; --jj)
#pragma unroll
      for (int cb = 0; cb < Q::KB1; ++cb) Rr[jj][cb] = duo_load_act<H, K, M, METHOD>(s0, jj, cb);
#pragma unroll
    for (int cb = 0; cb < Q::HB1; ++cb) Ry[cb] = duo_load_y<H, K, M, METHOD>(s0, cb, N, tile);
  }
  const bool trow = (lane & 3) == (H & 3);                 // lanes of the time row inside its column block H >> 2
  for (int e = 0; e < E; ++e) {
    // the chain wave has posted evaluation e (and is free to start e + 1).  No fence: an acquire would drain vmcnt and
    // with it the operand loads issued a whole evaluation ahead; LDS reads behind the barrier see the posted tiles.
    asm volatile("s_barrier" ::: "memory");
    const double* q = qbuf + (e & 1) * P::BUF;
    const Src sn(Y, act, tf, e + 1 < E ? e + 1 : e, L, N, tile);   // (the last evaluation reloads its own operands: no branch)
    // all A operands of the evaluation first (distinct registers, issued back to back: one exposed LDS latency per
    // evaluation), then block by block the matrix instructions and right behind them the reloads for the next evaluation
    double Ao[Q::HB], Az[M][Q::KB];
#pragma unroll
    for (int rb = 0; rb < Q::HB; ++rb) Ao[rb] = duo_readA(q + P::off(rb >> 2), rb & 3);
#pragma unroll
    for (int tq = 0; tq < M; ++tq)
#pragma unroll
      for (int rb = 0; rb < Q::KB; ++rb) Az[tq][rb] = duo_readA(q + P::off(D::HT + tq), rb);
    __builtin_amdgcn_sched_barrier(0);
    // cot(out) against [tanh ; 1]
#pragma unroll
    for (int cb = 0; cb < Q::KB1; ++cb)
#pragma unroll
      for (int rb = 0; rb < Q::HB; ++rb) gWo[rb][cb] = XW_MFMA4(Ao[rb], Ra[cb], gWo[rb][cb]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int cb = 0; cb < Q::KB1; ++cb) Ra[cb] = duo_load_act<H, K, M, METHOD>(sn, M - 1, cb);
    __builtin_amdgcn_sched_barrier(0);
    // cot(z_{j+1}) against [relu(z_j) ; 1], j = M-2 .. 0 (tile order of the chain wave)
#pragma unroll
    for (int jj = M - 2; jj >= 0; --jj) {
#pragma unroll
      for (int cb = 0; cb < Q::KB1; ++cb)
#pragma unroll
        for (int rb = 0; rb < Q::KB; ++rb) gWh[rb][cb] = XW_MFMA4(Az[M - 2 - jj][rb], Rr[jj][cb], gWh[rb][cb]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int cb = 0; cb < Q::KB1; ++cb) Rr[jj][cb] = duo_load_act<H, K, M, METHOD>(sn, jj, cb);
      __builtin_amdgcn_sched_barrier(0);
    }
    // cot(z_0) against [y_in ; t]: column H of dWy (the time row) is the time-column gradient
#pragma unroll
    for (int cb = 0; cb < Q::HB1; ++cb) {
      const double b = (cb == (H >> 2) && trow) ? ti_cur : Ry[cb];
#pragma unroll
      for (int rb = 0; rb < Q::KB; ++rb) gWy[rb][cb] = XW_MFMA4(Az[M - 1][rb], b, gWy[rb][cb]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int cb = 0; cb < Q::HB1; ++cb) Ry[cb] = duo_load_y<H, K, M, METHOD>(sn, cb, N, tile);
    __builtin_amdgcn_sched_barrier(0);
    ti_cur = sn.ti;
  }
  // ---- fold the path groups and store this tile's slab pieces: lane j + 16 i of block (rb, cb) holds (4 rb + i, 4 cb + j)
  double* slab = jobs.gslab[job] + (long)tile * o.total;
  const int i = lane >> 4, j = lane & 3;
  const bool owner = ((lane >> 2) & 3) == 0;
#pragma unroll
  for (int rb = 0; rb < Q::KB; ++rb)
#pragma unroll
    for (int cb = 0; cb < Q::KB1; ++cb) {
      const double x = duo_fold(gWh[rb][cb]);
      const int row = 4 * rb + i, col = 4 * cb + j;
      if (owner && row < K) {
        if (col < K) slab[o.Wh + row * K + col] = x;
        else if (col == K) slab[o.Whb + row] = x;
      }
    }
#pragma unroll
  for (int rb = 0; rb < Q::HB; ++rb)
#pragma unroll
    for (int cb = 0; cb < Q::KB1; ++cb) {
      const double x = duo_fold(gWo[rb][cb]);
      const int row = 4 * rb + i, col = 4 * cb + j;
      if (owner && row < H) {
        if (col < K) slab[o.Wo + row * K + col] = x;
        else if (col == K) slab[o.Wob + row] = x;
      }
    }
#pragma unroll
  for (int rb = 0; rb < Q::KB; ++rb)
#pragma unroll
    for (int cb = 0; cb < Q::HB1; ++cb) {
      const double x = duo_fold(gWy[rb][cb]);
      const int row = 4 * rb + i, col = 4 * cb + j;
      if (owner && row < K) {
        if (col < H) slab[o.Win + row * o.ldin + d + 1 + col] = x;
        else if (col == H) slab[o.Win + row * o.ldin + d] = x;
      }
    }
}

}  // namespace
