// xw_ode_mfma16.h -- the stepper's field on v_mfma_f64_16x16x4: the form of the WIDE container (64, 16), selected by -DXW_ODE_WIDE16
// (round 6).  Whole 16-row tiles, bias gradients as row sums -- no ones row, no 4x4 blocks, no narrow tiles; a duo sweep of its own.
// Included once: the field (operands, evaluation, vector-Jacobian product, gradient accumulators, the duo sweep's LDS plan), then
// storing the gradients and the duo sweep's second wave.
#pragma once
#include "xw_ode_core.h"

namespace {

static_assert(XW_ODE_K == 16 && XW_ODE_H % 16 == 0 && XW_ODE_H <= 64, "the wide container: K = 16, H a multiple of 16 up to 64");
// K = 16 and H = 16 HT are whole 16-row tiles, so the 16x16x4 form wastes nothing (at K = 10 it ran 10 of 16 rows): a [K x K]
// layer is 4 chained instructions, Win's y-part H / 4, Wo HT x 4.  An A-fragment is ONE double per lane and (tile, k-step):
// 16 + 4 + 4 HT doubles hold the whole field (as 4x4 blocks replicated over the lane blocks it would be 144 doubles at (64, 16)).
template <int H, int K> struct FieldW {
  double Wy[Dim<H, K>::KSH];                   // Win[:, d+1:]  [K x H], k-steps over H
  double Wh[Dim<H, K>::KSK];                   // Wh            [K x K]
  double Wo[Dim<H, K>::HT][Dim<H, K>::KSK];    // Wo            [H x K], row tiles x k-steps over K
  d4 wt, bh;
  d4 bo[Dim<H, K>::HT];
};
template <int H, int K> struct FieldWT {
  double WoT[Dim<H, K>::KSH];                  // (Wo^T) [K x H]
  double WhT[Dim<H, K>::KSK];                  // (Wh^T) [K x K]
  double WyT[Dim<H, K>::HT][Dim<H, K>::KSK];   // (Wy^T) [H x K]
};
template <int H, int K>
__device__ __forceinline__ void load_field(const double* __restrict__ th, const UOff& o, int d, FieldW<H, K>& w) {
  typedef Dim<H, K> D;
  const double* Wy = th + o.Win + d + 1;
#pragma unroll
  for (int ks = 0; ks < D::KSH; ++ks) w.Wy[ks] = xw_fragA(Wy, o.ldin, K, H, 0, 4 * ks);
#pragma unroll
  for (int ks = 0; ks < D::KSK; ++ks) w.Wh[ks] = xw_fragA(th + o.Wh, K, K, K, 0, 4 * ks);
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) {
#pragma unroll
    for (int ks = 0; ks < D::KSK; ++ks) w.Wo[ht][ks] = xw_fragA(th + o.Wo, K, H, K, 16 * ht, 4 * ks);
    w.bo[ht] = xw_vecD(th + o.Wob, H, 16 * ht);
  }
  w.wt = xw_vecD_strided(th + o.Win + d, o.ldin, K, 0);
  w.bh = xw_vecD(th + o.Whb, K, 0);
}
template <int H, int K>
__device__ __forceinline__ void load_field_T(const double* __restrict__ th, const UOff& o, int d, FieldWT<H, K>& w) {
  typedef Dim<H, K> D;
  const double* Wy = th + o.Win + d + 1;
#pragma unroll
  for (int ks = 0; ks < D::KSH; ++ks) w.WoT[ks] = xw_fragAT(th + o.Wo, K, H, K, 0, 4 * ks);          // (Wo^T)[i][4 ks + k] = Wo[4 ks + k][i]
#pragma unroll
  for (int ks = 0; ks < D::KSK; ++ks) w.WhT[ks] = xw_fragAT(th + o.Wh, K, K, K, 0, 4 * ks);
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht)
#pragma unroll
    for (int ks = 0; ks < D::KSK; ++ks) w.WyT[ht][ks] = xw_fragAT(Wy, o.ldin, K, H, 16 * ht, 4 * ks);   // (Wy^T)[16 ht + i][4 ks + k] = Wy[4 ks + k][16 ht + i]
}

template <int H, int K, int M, bool OUT = true, class Sink>
__device__ __forceinline__ void field_fwd(const FieldW<H, K>& w, double t, d4 xp, const d4 (&y)[Dim<H, K>::HT],
                                          d4 (&out)[Dim<H, K>::HT], const Sink& sink) {
  typedef Dim<H, K> D;
  d4 z;
#pragma unroll
  for (int r = 0; r < 4; ++r) z[r] = fma(w.wt[r], t, xp[r]);
#pragma unroll
  for (int ks = 0; ks < D::KSH; ++ks) z = XW_MFMA(w.Wy[ks], y[ks >> 2][ks & 3], z);
#pragma unroll
  for (int j = 0; j < M - 1; ++j) {
    d4 r;
#pragma unroll
    for (int kb = 0; kb < D::KB; ++kb) r[kb] = sink.relu(j, kb, z[kb]);
    sink.fence();
    sink.z(j, r);
    d4 nz = w.bh;
#pragma unroll
    for (int ks = 0; ks < D::KSK; ++ks) nz = XW_MFMA(w.Wh[ks], r[ks], nz);
    z = nz;
  }
  d4 a;
#pragma unroll
  for (int kb = 0; kb < D::KB; ++kb) a[kb] = xw_tanh(z[kb]);
  sink.a(a);
  if (!OUT) return;
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) {
    out[ht] = w.bo[ht];
#pragma unroll
    for (int ks = 0; ks < D::KSK; ++ks) out[ht] = XW_MFMA(w.Wo[ht][ks], a[ks], out[ht]);
  }
}

// parameter-gradient accumulators of the field (chain-layout tiles of the gradient matrices)
template <int H, int K> struct FieldG {           // wide container: no ones row / time row -- their gradients are elementwise sums
  d4 Wh;                                          // rows K, cols K
  d4 Wy[Dim<H, K>::CT];                           // rows K, cols H (tiles 0 .. HT-1; the last entry is not used)
  d4 Wo[Dim<H, K>::HT];                           // rows H, cols K
  // (these sums start at zero by their initialisers; sweep_body clears the three matrices, which both forms have)
  d4 bh = {}, wt = {};                            // sum over evaluations of cot(z_{j+1}) (Wh.b) and of t cot(z_0) (Win's time column), per path
  d4 bo[Dim<H, K>::HT] = {};                      // ... of cot(out) (Wo.b)
};
// (wide container: every Q tile is a full 16-row tile of the 16x16x4 form -- cot(out) x HT, cot(z_{j+1}) for j = M-2 .. 0, cot(z_0))
template <int H, int K, int M> struct DuoPlan {
  static constexpr int HT = Dim<H, K>::HT;
  static constexpr int NQ = HT + M;
  __device__ static constexpr int off(int t) { return t * XW_TTILE; }
  static constexpr int BUF = NQ * XW_TTILE;
  static_assert(BUF >= 3 * XW_TTILE, "the chain wave's epilogue borrows a buffer for its three transpose tiles");
};
template <int H, int K, int M, int OUTER, class SV>
__device__ __forceinline__ void field_vjp(const FieldW<H, K>& w, const FieldWT<H, K>& wT, double t, const SV& sv,
                                          const d4 (&yin)[Dim<H, K>::HT], const d4 (&ob)[Dim<H, K>::HT],
                                          d4 (&yb)[Dim<H, K>::HT], d4& xpb, FieldG<H, K>& G, double* lds) {
  typedef Dim<H, K> D;
  // OUTER: 0 = no weight gradients, 1 = this wave forms them itself (one LDS round trip per product, in the middle of the chain: the
  // recomputing sweeps), 2 = duo sweep: this wave only posts its cotangent tiles (transposed) into `lds` = the evaluation's Q buffer
  // (DuoPlan), the partner wave of the block (duo_outer) contracts them with the layer inputs it loads from the activation store
  constexpr bool PARAMS = OUTER == 1;
  constexpr bool POST = OUTER == 2;
  typedef DuoPlan<H, K, M> P;
  if (POST) {
#pragma unroll
    for (int ht = 0; ht < D::HT; ++ht) xw_writeT_n<4>(lds + P::off(ht), ob[ht]);
  }
  // cotangent of tanh(z_{m-1}): Wo^T cot(out), one chained accumulator over H / 4 k-steps
  d4 ab = xw_zero4();
#pragma unroll
  for (int ks = 0; ks < D::KSH; ++ks) ab = XW_MFMA(wT.WoT[ks], ob[ks >> 2][ks & 3], ab);
  if (PARAMS) {
    // dWo[16 ht ..][:] += cot(out)[ht] (x) tanh(z_{m-1}) over the 16 paths (LDS transposes, 4 k-steps each); dWo.b elementwise
#pragma unroll
    for (int ht = 0; ht < D::HT; ++ht) {
      outer_acc(G.Wo[ht], ob[ht], sv.a, lds);
      G.bo[ht] = G.bo[ht] + ob[ht];
    }
  }
  d4 zb;
#pragma unroll
  for (int r = 0; r < 4; ++r) zb[r] = ab[r] * (1.0 - sv.a[r] * sv.a[r]);
#pragma unroll
  for (int j = M - 2; j >= 0; --j) {
    if constexpr (PARAMS) {
      outer_acc(G.Wh, zb, sv.z[j], lds);
      G.bh = G.bh + zb;
    }
    if (POST) xw_writeT_n<4>(lds + P::off(D::HT + (M - 2 - j)), zb);      // cot(z_{j+1})
    d4 tt = xw_zero4();
#pragma unroll
    for (int ks = 0; ks < D::KSK; ++ks) tt = XW_MFMA(wT.WhT[ks], zb[ks], tt);
#pragma unroll
    for (int r = 0; r < 4; ++r) zb[r] = sv.gate(j, r, tt[r]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) xpb[r] += zb[r];
  if (POST) xw_writeT_n<4>(lds + P::off(D::HT + M - 1), zb);              // cot(z_0)
  if (PARAMS) {
#pragma unroll
    for (int ct = 0; ct < D::HT; ++ct) outer_acc(G.Wy[ct], zb, yin[ct], lds);
#pragma unroll
    for (int r = 0; r < 4; ++r) G.wt[r] = fma(t, zb[r], G.wt[r]);
  }
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) {
    yb[ht] = xw_zero4();
#pragma unroll
    for (int ks = 0; ks < D::KSK; ++ks) yb[ht] = XW_MFMA(wT.WyT[ht][ks], zb[ks], yb[ht]);
  }
}

// ---- the field gradients: into the slab; the duo sweep's second wave
// the field's weight-gradient accumulators -> one slab (wide container: the biases and the time column are row sums over the 16 paths)
template <int H, int K, bool HID = true, bool IO = true>
__device__ __forceinline__ void store_field_grads(double* slab, const UOff& o, int d, const FieldG<H, K>& G) {
  typedef Dim<H, K> D;
  const int lane = xw_lane(), g = lane >> 4;
  if (HID) {
    storeD(slab + o.Wh, K, K, K, 0, 0, G.Wh);
    storeRowSums(slab + o.Whb, K, 0, G.bh);
  }
  if (!IO) return;
#pragma unroll
  for (int ct = 0; ct < D::HT; ++ct) storeD(slab + o.Win + d + 1, o.ldin, K, H, 0, 16 * ct, G.Wy[ct]);
#pragma unroll
  for (int r = 0; r < 4; ++r) {                               // Win[:, d]: the time column
    const double s_ = xw_sum_over_n(G.wt[r]);
    const int row = g + 4 * r;
    if ((lane & 15) == 0 && row < K) slab[o.Win + (long)row * o.ldin + d] = s_;
  }
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) {
    storeD(slab + o.Wo, K, H, K, 16 * ht, 0, G.Wo[ht]);
    storeRowSums(slab + o.Wob, H, 16 * ht, G.bo[ht]);
  }
}
// ---- the duo sweep's second wave in the wide container: weight gradients of the field on v_mfma_f64_16x16x4 --------------------
// One wave that runs the adjoint chain AND its 15 outer products per evaluation paid an LDS round trip per product in the middle
// of the chain and spilled 330 registers (641 us per sweep at the headline sample against 161 us without weight gradients).  As in
// the narrow containers the chain wave only POSTS its cotangent tiles (field_vjp OUTER = 2: cot(out) x HT, cot(z_{j+1}) of every
// tied layer, cot(z_0); two alternating buffers, one s_barrier per evaluation) and this wave, one evaluation behind, contracts
// them over the 16 paths with the layer inputs it loads from the activation store / the checkpoints itself, a whole evaluation
// ahead: 4 (HT + M - 1 + HT) matrix instructions per evaluation.  A operand = xw_readT of a posted tile (row i, path 4 ks + kk);
// B operand = (row j, path 4 ks + kk) of a 16-row block of the record, whose 4-row blocks are path-major (act_store): double
// 64 (j >> 2) + 4 (4 ks + kk) + (j & 3) of the block.  The bias gradients and the time column are row sums of the posted tiles: a
// lane adds the A operands it reads anyway, the four lane groups are folded once at the end.
template <int H, int K, int M, int METHOD>
__device__ __forceinline__ void duo_outer(const BwdJobs& jobs, const double* __restrict__ tf, const double* __restrict__ th,
                                          int L, int d, const double* qbuf, int vb) {
  typedef Dim<H, K> D;
  typedef RK<METHOD> T;
  typedef DuoPlan<H, K, M> P;
  typedef ActLayout<H, K, M, T::S> AL;
  constexpr int NH = M > 1 ? M - 1 : 1;
  xw_setprio(jobs.prio);
  const int job = find_job(jobs, vb);
  const double* __restrict__ Y = jobs.Y[job];
  const double* __restrict__ act = jobs.act[job];
  const int N = jobs.N[job];
  const int tile = vb - jobs.tile0[job];
  const int lane = xw_lane(), j = lane & 15, kk = lane >> 4;
  const UOff o = u_offsets(d, H, K);
  const int lo = 64 * (j >> 2) + 4 * kk + (j & 3);
  const long ntile = (N + 15) >> 4;
  long ycol[4];                                          // columns of the checkpoint this lane reads (clamped: the last tile's padding paths)
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const long c = (long)tile * 16 + 4 * ks + kk;
    ycol[ks] = c < N ? c : N - 1;
  }
  d4 gWo[D::HT], gWy[D::HT], gWh = xw_zero4();
  double sbo[D::HT], sbh = 0.0, swt = 0.0;
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) {
    gWo[ht] = xw_zero4();
    gWy[ht] = xw_zero4();
    sbo[ht] = 0.0;
  }
  double Ra[4], Rr[NH][4], Ry[D::HT][4];                 // B operands of the evaluation in flight
  const int E = (L - 1) * T::S;                          // field evaluations of the sweep (chain-wave order: steps L-2 .. 0, stages S-1 .. 0)
  // operands of evaluation e: the record of its step, its stage, its time
  auto load_eval = [&](int e, double& ti) {
    const int l = L - 2 - e / T::S, i = T::S - 1 - e % T::S;
    const double* __restrict__ A = act + ((long)l * ntile + tile) * (AL::TOTAL * 16) + lo;
    const double t0 = tf[l];
    ti = t0 + T::c(i) * (tf[l + 1] - t0);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) Ra[ks] = __builtin_nontemporal_load(A + (i * AL::STAGE + (M - 1) * K) * 16 + 16 * ks);
#pragma unroll
    for (int jj = 0; jj < M - 1; ++jj)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) Rr[jj][ks] = __builtin_nontemporal_load(A + (i * AL::STAGE + jj * K) * 16 + 16 * ks);
    // the field's input: the checkpoint y_l [H][N] (stage 0) or the stage input kept in the record
    const bool first = i == 0;                           // (wave-uniform)
#pragma unroll
    for (int ct = 0; ct < D::HT; ++ct)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const double* __restrict__ sy = Y + ((long)l * H + 16 * ct + j) * N + ycol[ks];
        const double* __restrict__ sa = A + (long)(AL::YI + (i > 0 ? i - 1 : 0) * H + 16 * ct) * 16 + 16 * ks;
        Ry[ct][ks] = __builtin_nontemporal_load(first ? sy : sa);
      }
  };
  double ti_cur = 0.0;
  if (E > 0) load_eval(0, ti_cur);
  for (int e = 0; e < E; ++e) {
    // the chain wave has posted evaluation e (and is free to start e + 1).  No fence: an acquire would drain vmcnt and with it the
    // operand loads issued a whole evaluation ahead; LDS reads behind the barrier see the posted tiles.
    asm volatile("s_barrier" ::: "memory");
    const double* q = qbuf + (e & 1) * P::BUF;
    double Ao[D::HT][4], Az[M][4];
#pragma unroll
    for (int ht = 0; ht < D::HT; ++ht)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) Ao[ht][ks] = xw_readT(q + P::off(ht), ks);
#pragma unroll
    for (int tq = 0; tq < M; ++tq)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) Az[tq][ks] = xw_readT(q + P::off(D::HT + tq), ks);
    __builtin_amdgcn_sched_barrier(0);
    // cot(out) against tanh(z_{m-1})
#pragma unroll
    for (int ht = 0; ht < D::HT; ++ht) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) gWo[ht] = XW_MFMA(Ao[ht][ks], Ra[ks], gWo[ht]);
      sbo[ht] += (Ao[ht][0] + Ao[ht][1]) + (Ao[ht][2] + Ao[ht][3]);
    }
    // cot(z_{j+1}) against relu(z_j), j = M-2 .. 0 (tile order of the chain wave); the record keeps the layer INPUT z_j
#pragma unroll
    for (int jj = M - 2; jj >= 0; --jj) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const double r = Rr[jj][ks];
        gWh = XW_MFMA(Az[M - 2 - jj][ks], r, gWh);
      }
      sbh += (Az[M - 2 - jj][0] + Az[M - 2 - jj][1]) + (Az[M - 2 - jj][2] + Az[M - 2 - jj][3]);
    }
    // cot(z_0) against the field's input; its row sums times t are the time column
#pragma unroll
    for (int ct = 0; ct < D::HT; ++ct)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) gWy[ct] = XW_MFMA(Az[M - 1][ks], Ry[ct][ks], gWy[ct]);
    swt = fma(ti_cur, (Az[M - 1][0] + Az[M - 1][1]) + (Az[M - 1][2] + Az[M - 1][3]), swt);
    __builtin_amdgcn_sched_barrier(0);
    load_eval(e + 1 < E ? e + 1 : e, ti_cur);            // (the last evaluation reloads its own operands: no branch)
    __builtin_amdgcn_sched_barrier(0);
  }
  // ---- this tile's slab pieces: accumulator register r of lane (g, n) = element (row g + 4 r, column n)
  double* slab = jobs.gslab[job] + (long)tile * o.total;
  storeD(slab + o.Wh, K, K, K, 0, 0, gWh);                  // (u_layers = 1: zeros -- the slot of the missing tied layer)
#pragma unroll
  for (int ct = 0; ct < D::HT; ++ct) storeD(slab + o.Win + d + 1, o.ldin, K, H, 0, 16 * ct, gWy[ct]);
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) storeD(slab + o.Wo, K, H, K, 16 * ht, 0, gWo[ht]);
  // row sums: lane (row j, group kk) holds its group's share
  auto fold = [](double x) {
    x += __shfl_xor(x, 16);
    x += __shfl_xor(x, 32);
    return x;
  };
  sbh = fold(sbh);
  swt = fold(swt);
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) sbo[ht] = fold(sbo[ht]);
  if (kk == 0) {
    if (j < K) slab[o.Whb + j] = sbh;
    if (j < K) slab[o.Win + (long)j * o.ldin + d] = swt;
#pragma unroll
    for (int ht = 0; ht < D::HT; ++ht)
      if (16 * ht + j < H) slab[o.Wob + 16 * ht + j] = sbo[ht];
  }
}

}  // namespace
