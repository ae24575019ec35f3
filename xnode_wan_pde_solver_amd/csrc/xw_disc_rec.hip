// xw_disc_rec.hip -- adversarial test network v_phi on gfx950: the parameter gradient from the activation record (k_disc_rec, all
// 24 instantiations) and its launcher.  xw_disc_bwd (xw_disc_bwd.hip) is the entry point in front of it; xw_disc_core.h has the
// overview of the family.
#include "xw_disc_core.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// k_disc_rec: the parameter gradient from the activation record, two blocks per CU.
// k_disc_bwd (xw_disc_bwd.hip) needs 157 KB of LDS (one block per CU, one wave per SIMD: every barrier / transpose stall of that
// wave is idle matrix-pipe time).  This kernel only ever runs from the record, so
//   * the forward fragments of Vh are gone, and of Vh^T only the three full row tiles stay in LDS: rows 48, 49 of the
//     reverse chain (W = 50) are contracted on the vector ALU from a 104-double table, as in k_disc_fwd -- 39 instead of
//     52 chain MFMAs per layer;
//   * the last transposed tile of every set stores its one live 4-row group (rows 48..51) instead of 16 rows; operand
//     rows read past it (lane & 15 >= 4, folded back with & 3) only reach accumulator rows / columns that are never stored;
//   * the dVo partial sums are reduced over the 16 points of a tile before they go to LDS (256 instead of 4096 doubles);
//   * the input-layer gradient is contracted in groups of 48 input rows (three full tiles);
// -> 78 KB per block, <= 256 registers per wave: two blocks share a CU and cover each other's barriers.
#ifdef XW_REC_PROBE     // diagnostic build only (tools/probe_rec_phases.py): shader clocks per phase of every wave of k_disc_rec
__device__ unsigned long long xw_rec_clock[12 * 2048];
#define XW_PH(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); phc[i] += t_ - phl; phl = t_; }
#else
#define XW_PH(i)
#endif
template <int W> struct RecLds {
  typedef VDim<W> D;
  // W = 49..51: short last row tile -- vector-ALU tail + one live 4-row group, 78 KB, two blocks per CU.  Otherwise
  // (W = 64, the container of the widths above 50) four full tiles everywhere: 105 KB, one block per CU.
  static constexpr bool VT = D::VTAIL;
  static_assert(!VT || D::LR(D::MT - 1) == 1, "short last row tile: vector-ALU tail + one live 4-row group");
  static constexpr int T3 = VT ? 4 * XW_TSTRIDE : XW_TTILE;       // trimmed last tile
  static constexpr int wset = (D::MT - 1) * XW_TTILE + T3;        // one wave's set of transposed tiles
  // W = 128: the 131 KB of Vh^T fragments do not fit beside the tile sets (139 KB) -- the reverse chain takes them from L2,
  // one k-step ahead, like the fused input gradient of k_disc_fwd
  static constexpr bool FRAG_LDS = D::MT == 4;
  static constexpr int oVhT = 0;                                  // [MTF][KS][64]
  static constexpr int oTT = oVhT + (FRAG_LDS ? D::MTF * D::KS * 64 : 0);   // [4 KS][TR]: Vh[k][16 (MT-1) + r]
  static constexpr int oVo = oTT + (VT ? 4 * D::KS * D::TR : 0);  // Vo, zero-padded to 16 MT rows
  static constexpr int oD = oVo + 16 * D::MT;
  static constexpr int oR = oD + 4 * wset;
  static constexpr int oO = oR + 4 * wset;                        // [4 MT row slots + dVo.b][4 waves][4 g]
  static constexpr int NO = 4 * D::MT;                            // row slots of dVo
  static constexpr int total = oO + (NO + 1) * 16;
  static_assert(total * 8 <= (VT ? 80 : 160) * 1024, "two blocks per CU (short tail) / one");
  __device__ static constexpr int toff(int mt) { return mt * XW_TTILE; }
};

// operand read from a wave's tile set: tile mt, folded back into the live rows when it is the trimmed one
template <int W> __device__ __forceinline__ double rec_readT(const double* set, int mt, int ks) {
  const int l = xw_lane();
  const int row = (RecLds<W>::VT && mt == VDim<W>::MT - 1) ? (l & 3) : (l & 15);
  return set[RecLds<W>::toff(mt) + row * XW_TSTRIDE + 4 * ks + (l >> 4)];
}

// TSUM (path mode, N a multiple of 64: every 64-point unit is 64 consecutive paths at ONE time index): the input layer's
//   gradient dVin = sum_p delta_0[p] (x) [t_p ; x_p ; 1] is not contracted unit by unit.  A block takes a CONTIGUOUS run of units in
//   (path group, time index) order -- its waves stay on the same 16 paths while the time index advances -- and x does not move
//   along a vertical path, so  dVin[:, 1..d] = (sum_l delta_0) (x) x,  dVin.b = rowsum(sum_l delta_0),  dVin[:, 0] = rowsum(sum_l
//   t_l delta_0):  two running sums in registers per unit (26 multiply-adds) and ONE contraction per path group instead of one
//   per unit (per unit it was 12 gathered loads, 12 LDS stores, two barriers, 32 matrix instructions and a read-modify-write of
//   the slab: 11 % of a wave's time, profiles/r04_probe_rec_phases.txt).
template <int W, int Q, int NG, bool TSUM>
__global__ void __launch_bounds__(256, RecLds<W>::VT ? 2 : 1) k_disc_rec(const double* __restrict__ xT, const double* __restrict__ tf,
                                                     const double* __restrict__ tpp, const double* __restrict__ ph,
                                                     const double* __restrict__ vbar, int N, int L, int d,
                                                     double* __restrict__ gslab, const double* __restrict__ act, int qrt) {
  typedef VDim<W> D;
  typedef RecLds<W> S;
  __shared__ double lds[S::total];
  double* sVhT = lds + S::oVhT;
  double* sTT = lds + S::oTT;
  double* sVo = lds + S::oVo;
  double* sO = lds + S::oO;
  const int lane = xw_lane(), g = lane >> 4, n = lane & 15;
  const int wave = threadIdx.x >> 6;
  double* myD = lds + S::oD + wave * S::wset;
  double* myR = lds + S::oR + wave * S::wset;
#ifdef XW_REC_PROBE
  const unsigned long long ck_in = __builtin_amdgcn_s_memtime(), rt_in = __builtin_amdgcn_s_memrealtime();
#endif
  const VOff o = v_offsets(d, W);
  const long P = (long)N * L;
  const long nsuper = (P + 63) / 64;
  const int nq = Q > 0 ? Q : qrt;
  constexpr int UNROLL = Q > 0 ? Q : 1;
  constexpr int TW = D::MT / 2;                      // 2 x 2 waves x TW x TW tiles of dVh
  const int wi = wave >> 1, wj = wave & 1;

  if (S::FRAG_LDS)
    for (int idx = wave; idx < D::MTF * D::KS; idx += 4) {
      const int mt = idx / D::KS, ks = idx - mt * D::KS;
      sVhT[idx * 64 + lane] = xw_fragAT(ph + o.Vh, W, W, W, 16 * mt, 4 * ks);
    }
  if (S::VT)
    for (int idx = threadIdx.x; idx < 4 * D::KS * D::TR; idx += blockDim.x) {
      const int r = idx % D::TR, k = idx / D::TR;                        // reverse chain: nd[48 + r] = sum_k Vh[k][48 + r] dl[k]
      sTT[idx] = k < W ? ph[o.Vh + (long)k * W + 16 * (D::MT - 1) + r] : 0.0;
    }
  if (threadIdx.x < 16 * D::MT) sVo[threadIdx.x] = (int)threadIdx.x < W ? ph[o.Vo + threadIdx.x] : 0.0;
  for (int idx = threadIdx.x; idx < (S::NO + 1) * 16; idx += blockDim.x) sO[idx] = 0.0;
  __syncthreads();

  d4 accH[TW * TW], accB[D::MT];                     // accB: dVh.b without the ones row (W a multiple of 16)
#pragma unroll
  for (int ct = 0; ct < TW * TW; ++ct) accH[ct] = xw_zero4();
#pragma unroll
  for (int ct = 0; ct < D::MT; ++ct) accB[ct] = xw_zero4();
  // ---- short last row tile (W = 50): dVh = 48 x 48 core on 16x16x4 tiles + the two edges on 4x4x4 blocks.
  // As 4 x 4 tiles of 16 x 16 the outer products ran 16 matrix instructions per k-step for 50 x 51 live entries of 64 x 64
  // (61 %): 7 of the 16 tiles existed for rows 48, 49 / columns 48..50.  Now, per 16 points,
  //     core  : 9 tiles x 4 k-steps of 66 clocks -- two tiles per wave (accH[0], accH[1]) and tile (2, 2) of the wave's OWN
  //             16 points (accH[2]: a partial sum per wave, needs no barrier; the four are added once, at the end);
  //     edges : rows 48..51 x column blocks 0..12 (waves 0, 1) and row blocks 0..11 x columns 48..51 (waves 2, 3) as
  //             v_mfma_f64_4x4x4 -- the instruction's four blocks are the four groups of four points, so ONE instruction
  //             is a 4 x 4 block of dVh over all 16 points (18 clocks; the four partials are folded once, at the end).
  //             The column edge is computed transposed (A = input rows 48..51, B = cotangent rows), so that all four waves
  //             run the same code: one fixed operand X, 6-7 varying operands V.
  // 2826 instead of 4224 matrix clocks per 16 points and layer, 706 +- 14 per wave.
  constexpr bool EDGE = S::VT;
  constexpr int NE = 7;
  double accE[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) accE[e] = 0.0;
  // core tiles: waves 0..2 row band `wave` x column tiles 0, 1 (one cotangent operand, two input operands per k-step); wave 3
  // column tile 2 x row bands 0, 1, computed transposed (A = input tile 2, B = the two cotangent tiles): three operand
  // reads per two matrix instructions in every wave, the same code in all of them
  const int vstart = wave == 1 ? 7 : wave == 3 ? 6 : 0;
  const int lane16 = (lane & 15) * XW_TSTRIDE + (lane >> 4);                       // 16x16x4 operand: row i, point 4 ks + k
  const int lane4 = (lane & 3) * XW_TSTRIDE + ((lane >> 2) & 3) * 4 + (lane >> 4);  // 4x4x4 operand: row i, point 4 blk + k
  const int offC = (wave < 3 ? S::oD + wave * XW_TTILE : S::oR + 2 * XW_TTILE) + lane16;
  const int offW = (wave < 3 ? S::oR : S::oD) + lane16;
  const int offX = (wave < 2 ? S::oD : S::oR) + 48 * XW_TSTRIDE + lane4;
  const int offV = (wave < 2 ? S::oR : S::oD) + vstart * 4 * XW_TSTRIDE + lane4;
  double* slab = gslab + (long)blockIdx.x * o.total;

#ifdef XW_REC_PROBE
  unsigned long long phc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, phl = __builtin_amdgcn_s_memtime();
#endif
  // TSUM: this block's units [u0, u1) in (path group, time index) order; unit u = (ng, l) is super-tile l (N / 64) + ng
  const long ngs = N >> 6;
  const long ub = nsuper / gridDim.x, ur = nsuper % gridDim.x;
  const long u0 = (long)blockIdx.x * ub + ((long)blockIdx.x < ur ? (long)blockIdx.x : ur), u1 = u0 + ub + ((long)blockIdx.x < ur ? 1 : 0);
  d4 sumS[D::MT], sumT[D::MT];                       // TSUM: sum_l delta_0, sum_l t_l delta_0 of the current path group
#pragma unroll
  for (int mt = 0; mt < D::MT; ++mt) sumS[mt] = sumT[mt] = xw_zero4();
  bool slab_first = true;                            // (uniform) the block's slab has not been written yet
  for (long it = TSUM ? u0 : (long)blockIdx.x; it < (TSUM ? u1 : nsuper); it += TSUM ? 1 : (long)gridDim.x) {
    const long ung = TSUM ? it / L : 0;
    const long st = TSUM ? (it - ung * L) * ngs + ung : it;
    const Pt pt = locate(st * 4 + wave, P, N, tf, tpp);
    // tile-major record (see k_disc_fwd): this wave's tile is one contiguous stretch, a layer 13 x 512 contiguous bytes
    const long ntile = (P + 15) >> 4;
    const long tl = st * 4 + wave < ntile ? st * 4 + wave : ntile - 1;  // (a wave past the end re-reads the last tile; vb = 0)
    const double* tbase = act + (long)__builtin_amdgcn_readfirstlane((int)tl) * ((long)(nq + 1) * W * 16);
    const int aoff = lane;
    auto load_layer = [&](int j, d4 (&r)[D::MT]) {
      const double* base = tbase + j * W * 16;
      asm volatile("" : "+s"(base));
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
        for (int q_ = 0; q_ < 4; ++q_)
          if (q_ < D::LR(mt)) {
            const int row = 16 * mt + 4 * q_ + g;
            r[mt][q_] = (16 * mt + 4 * q_ + 3 < W || row < W) ? xw_ld_nt(base + (16 * mt + 4 * q_) * 16 + aoff) : 0.0;
          }
    };
    // (requesting the first two layers of the NEXT tile in front of this tile's input-layer gradient, so that a tile does not
    //  start with a round trip to memory: 13 spilled registers, no gain -- the other wave of the SIMD covers that wait)
    d4 a[D::MT], rnext[D::MT];
    load_layer(nq, a);                                 // tanh(a_q)
    if (nq > 0) load_layer(nq - 1, rnext);
    const double vb = pt.valid ? (vbar != nullptr ? xw_ld_g(vbar + pt.p) : 1.0) : 0.0;
    // ---- output layer: cotangent of a_q, and dVo / dVo.b reduced over the 16 points of the tile
    d4 dl[D::MT];
#pragma unroll
    for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (r < D::LR(mt) && 16 * mt + 4 * r < W) {
          const double th = a[mt][r];
          dl[mt][r] = sVo[16 * mt + g + 4 * r] * (1.0 - th * th) * vb;
          const double s_ = xw_sum_over_n(vb * th);
          if (n == 0) sO[(mt * 4 + r) * 16 + wave * 4 + g] += s_;
        } else {
          dl[mt][r] = 0.0;
        }
      }
    {
      const double s_ = xw_sum_over_n(vb);
      if (lane == 0) sO[S::NO * 16 + wave * 4] += s_;
    }
    XW_PH(6)
    // ---- reverse chain, one layer at a time; the next layer's inputs are in flight meanwhile
#pragma unroll UNROLL
    for (int sg = nq - 1; sg >= 0; --sg) {
      // the layer's inputs are only needed transposed in LDS and, afterwards, as the ReLU mask: 13 sign bits, not 26 registers
      bool open[4 * D::MT];                           // (lane masks in scalar register pairs: one compare now, one select later)
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) open[4 * mt + r] = r < D::LR(mt) && rnext[mt][r] > 0.0;
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt) {
        d4 rr = rnext[mt];
        if (D::BIASROW && mt == (W >> 4)) {
          if (g == ((W & 15) & 3)) rr[(W & 15) >> 2] = 1.0;            // ones row -> column W of dVh collects dVh.b
        }
        if (!D::BIASROW) accB[mt] = accB[mt] + dl[mt];
        if (mt < D::MT - 1 || !S::VT) {
          xw_writeT(myD + S::toff(mt), dl[mt]);
          xw_writeT(myR + S::toff(mt), rr);
        } else {
          xw_writeT_n<1>(myD + S::toff(mt), dl[mt]);
          xw_writeT_n<1>(myR + S::toff(mt), rr);
        }
      }
      if (sg > 0) load_layer(sg - 1, rnext);                           // in flight while this layer is reversed
      XW_PH(0)
      // reverse chain: three row tiles on the matrix pipe, rows 16 (MT-1) + r on the vector ALU
      d4 nd[D::MT];
      asm volatile("" ::: "memory");
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt) nd[mt] = xw_zero4();
      double tv[D::TR];
#pragma unroll
      for (int r = 0; r < D::TR; ++r) tv[r] = 0.0;
      if constexpr (S::FRAG_LDS) {
#pragma unroll
        for (int ks = 0; ks < D::KS; ++ks) {
          const double b = dl[ks >> 2][ks & 3];
          if ((ks & 1) == 0) asm volatile("" ::: "memory");   // bound the LDS loads in flight (else they are all hoisted -> spills)
#pragma unroll
          for (int mt = 0; mt < D::MTF; ++mt) nd[mt] = XW_MFMA(sVhT[(mt * D::KS + ks) * 64 + lane], b, nd[mt]);
          if (S::VT) {
#pragma unroll
            for (int r = 0; r < D::TR; ++r) tv[r] = fma(sTT[(4 * ks + g) * D::TR + r], b, tv[r]);
          }
        }
      } else {
        // the wide container: Vh^T fragments from L2, requested one k-step ahead (laundered base and lane id: the per-lane
        // fragment addresses are formed here, not hoisted out of the tile loop into spilled registers)
        const double* phg = ph;
        int ll = lane;
        asm volatile("" : "+s"(phg), "+v"(ll));
        double fn[D::MT];
#pragma unroll
        for (int mt = 0; mt < D::MT; ++mt) fn[mt] = xw_fragAT_l(phg + o.Vh, W, W, W, 16 * mt, 0, ll);
#pragma unroll
        for (int ks = 0; ks < D::KS; ++ks) {
          const double b = dl[ks >> 2][ks & 3];
          double fc[D::MT];
#pragma unroll
          for (int mt = 0; mt < D::MT; ++mt) fc[mt] = fn[mt];
          if (ks + 1 < D::KS) {
#pragma unroll
            for (int mt = 0; mt < D::MT; ++mt) fn[mt] = xw_fragAT_l(phg + o.Vh, W, W, W, 16 * mt, 4 * (ks + 1), ll);
          }
          asm volatile("" ::: "memory");
#pragma unroll
          for (int mt = 0; mt < D::MT; ++mt) nd[mt] = XW_MFMA(fc[mt], b, nd[mt]);
        }
      }
      if (S::VT) {
#pragma unroll
        for (int r = 0; r < D::TR; ++r) {
          const double s_ = xw_sum_over_g(tv[r]);
          if (g == r) nd[D::MT - 1][0] = s_;
        }
      }
      XW_PH(1)
      if (EDGE) {
        // tile (2, 2) over the wave's own points: its own transposed tiles, no barrier needed
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          accH[2] = XW_MFMA(xw_readT(myD + S::toff(2), ks), xw_readT(myR + S::toff(2), ks), accH[2]);
      }
      XW_PH(2)
      __syncthreads();
      XW_PH(3)
      if (EDGE) {
#pragma unroll
        for (int pw = 0; pw < 4; ++pw) {
          const double* set = lds + pw * S::wset;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            if ((ks & 1) == 0) asm volatile("" ::: "memory");
            const double xc = set[offC + 4 * ks], w0 = set[offW + 4 * ks], w1 = set[offW + XW_TTILE + 4 * ks];
            accH[0] = XW_MFMA(xc, w0, accH[0]);
            accH[1] = XW_MFMA(xc, w1, accH[1]);
          }
          asm volatile("" ::: "memory");
          const double x = set[offX];
#pragma unroll
          for (int e = 0; e < NE; ++e)
            if (e < NE - 1 || wave == 0) accE[e] = XW_MFMA4(x, set[offV + e * 4 * XW_TSTRIDE], accE[e]);
        }
      } else {
#pragma unroll
        for (int pw = 0; pw < 4; ++pw) {
          const double* setD = lds + S::oD + pw * S::wset;
          const double* setR = lds + S::oR + pw * S::wset;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            if ((ks & 1) == 0) asm volatile("" ::: "memory");
            // TW x TW tiles of dVh per wave: 2 TW operand reads feed TW^2 MFMAs (2 x 2: four reads, four MFMAs; 4 x 4: eight, sixteen)
            double aa[TW], bb[TW];
#pragma unroll
            for (int i_ = 0; i_ < TW; ++i_) {
              aa[i_] = rec_readT<W>(setD, TW * wi + i_, ks);
              bb[i_] = rec_readT<W>(setR, TW * wj + i_, ks);
            }
#pragma unroll
            for (int i_ = 0; i_ < TW; ++i_)
#pragma unroll
              for (int j_ = 0; j_ < TW; ++j_) accH[i_ * TW + j_] = XW_MFMA(aa[i_], bb[j_], accH[i_ * TW + j_]);
          }
        }
      }
      XW_PH(4)
      __syncthreads();
      XW_PH(5)
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dl[mt][r] = open[4 * mt + r] ? nd[mt][r] : 0.0;
    }
    // ---- dl = cotangent of a_0.  Input layer: dVin = dl (x) [t; x; 1], 48 input rows at a time
    // contraction of a cotangent tile set Dm (chain layout) with the input rows of this wave's 16 points over the block's 64
    // points; rows: 0 = all of [t; x; 1] (one unit), 1 = [0; x; 1] (a path group's sum over the time indices), 2 = [1; 0; 0]
    // (the time column from the t-weighted sum).  acc0: what tile 0 of group 0 starts from; the result goes to the slab.
    constexpr int RH = (D::MT + 3) / 4;       // row tiles of dVin a wave owns: wave, wave + 4, ... (below MT)
    struct InAcc { d4 v[RH]; };
    auto contract_input = [&](const d4 (&Dm)[D::MT], const int rows, const InAcc& acc0, InAcc* keep0) {
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt) {
        if (mt < D::MT - 1 || !S::VT) xw_writeT(myD + S::toff(mt), Dm[mt]);
        else xw_writeT_n<1>(myD + S::toff(mt), Dm[mt]);
      }
      const double* xl = xT;                    // laundered: the per-lane row addresses of x and of the slab are formed here,
      double* sl = slab;                        // not hoisted out of the tile loop into (spilled) registers
      int gl = g, nl = n;                       // (and copies of the lane coordinates the compiler cannot see through)
      asm volatile("" : "+s"(xl), "+s"(sl), "+v"(gl), "+v"(nl));
#pragma unroll
      for (int grp = 0; grp < NG; ++grp) {
        if (rows == 2 && grp > 0) break;
        const int nct = rows == 2 ? 1 : (d + 2 - 48 * grp >= 33 ? 3 : d + 2 - 48 * grp >= 17 ? 2 : 1);     // live 16-row tiles of this group
#pragma unroll
        for (int rr = 0; rr < 12; ++rr) {
          if (rr >= 4 * nct) continue;
          const int cl = gl + 4 * rr;           // local row 0..47 of this group
          const int c = 48 * grp + cl;          // input row: 0 = t, 1..d = x, d+1 = ones
          double val = 0.0;
          if (pt.valid) {
            if (rows == 2) val = c == 0 ? 1.0 : 0.0;
            else if (c == 0) val = rows == 0 ? pt.t : 0.0;
            else if (c <= d) val = xw_ld_g(xl + (long)(c - 1) * N + pt.n);
            else if (c == d + 1) val = 1.0;
          }
          myR[S::toff(cl >> 4) + (cl & 15) * XW_TSTRIDE + nl] = val;
        }
        __syncthreads();
        d4 accIn[RH][3];
#pragma unroll
        for (int rh = 0; rh < RH; ++rh) {
#pragma unroll
          for (int ct = 0; ct < 3; ++ct) accIn[rh][ct] = xw_zero4();
          if (grp == 0) accIn[rh][0] = acc0.v[rh];
        }
#pragma unroll
        for (int pw = 0; pw < 4; ++pw) {
          const double* setD = lds + S::oD + pw * S::wset;
          const double* setR = lds + S::oR + pw * S::wset;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            double av[RH], bv[3];
#pragma unroll
            for (int rh = 0; rh < RH; ++rh) av[rh] = rec_readT<W>(setD, wave + 4 * rh < D::MT ? wave + 4 * rh : wave, ks);   // (a tile the wave does not own: a copy, never stored)
#pragma unroll
            for (int ct = 0; ct < 3; ++ct) bv[ct] = ct < nct ? rec_readT<W>(setR, ct, ks) : 0.0;
#pragma unroll
            for (int rh = 0; rh < RH; ++rh)
#pragma unroll
              for (int ct = 0; ct < 3; ++ct)
                if (ct < nct) accIn[rh][ct] = XW_MFMA(av[rh], bv[ct], accIn[rh][ct]);
          }
        }
        __syncthreads();
        if (keep0 != nullptr) {                 // (the time-column pass: its tiles are what the next pass starts from)
#pragma unroll
          for (int rh = 0; rh < RH; ++rh) keep0->v[rh] = accIn[rh][0];
          break;
        }
        // dVin is touched once per contraction: it is accumulated in the block's slab (L2), not in 24 registers per group that
        // would be live through every layer above.  Wave `wave` owns rows [16 wave, 16 wave + 16) (+ 64 in the wide container).
#pragma unroll
        for (int rh = 0; rh < RH; ++rh)
#pragma unroll
          for (int ct = 0; ct < 3; ++ct) {
            if (ct >= nct) continue;
            const int c = 48 * grp + 16 * ct + nl;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = 16 * (wave + 4 * rh) + gl + 4 * r;
              if (wave + 4 * rh < D::MT && row < W && c <= d + 1) {
                double* dst = c <= d ? sl + o.Vin + row * o.ldin + c : sl + o.Vinb + row;
                xw_st_g(slab_first ? accIn[rh][ct][r] : xw_ld_g(dst) + accIn[rh][ct][r], dst);
              }
            }
          }
      }
    };
    InAcc zacc;
#pragma unroll
    for (int rh = 0; rh < RH; ++rh) zacc.v[rh] = xw_zero4();
    if (!TSUM) {
      contract_input(dl, 0, zacc, nullptr);
      slab_first = false;
    } else {
      const double tl = pt.t;                   // (one time index per unit)
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (r < D::LR(mt)) {
            sumS[mt][r] += dl[mt][r];
            sumT[mt][r] = fma(tl, dl[mt][r], sumT[mt][r]);
          }
      if (it + 1 == u1 || (it + 1) / L != ung) {           // (uniform) the path group ends here: contract its sums
        InAcc tcol;
        contract_input(sumT, 2, zacc, &tcol);
        contract_input(sumS, 1, tcol, nullptr);
        slab_first = false;
#pragma unroll
        for (int mt = 0; mt < D::MT; ++mt) sumS[mt] = sumT[mt] = xw_zero4();
      }
    }
    XW_PH(7)
  }
#ifdef XW_REC_PROBE
  const unsigned long long ck_loop = __builtin_amdgcn_s_memtime();
#endif

  if (EDGE) {
    // core tiles: (row band wave, column tile t) / wave 3 transposed: (row band t, column tile 2)
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wave < 3 ? 16 * wave + g + 4 * r : 16 * t2 + n, c = wave < 3 ? 16 * t2 + n : 32 + g + 4 * r;
        slab[o.Vh + row * W + c] = accH[t2][r];
      }
    // tile (2, 2): the four waves' partial sums, through the idle tile area
    __syncthreads();
    double* s22 = lds + S::oD;
#pragma unroll
    for (int r = 0; r < 4; ++r) s22[wave * 256 + (g + 4 * r) * 16 + n] = accH[2][r];
    __syncthreads();
    {
      const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
      slab[o.Vh + (32 + i) * W + 32 + j] = (s22[threadIdx.x] + s22[256 + threadIdx.x]) + (s22[512 + threadIdx.x] + s22[768 + threadIdx.x]);
    }
    // edges: fold the four point groups (lane bits 2, 3); lane j + 16 i of group 0 holds entry (i, j) of the block
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      double s_ = accE[e];
      s_ += __shfl_xor(s_, 4);
      s_ += __shfl_xor(s_, 8);
      if ((e < NE - 1 || wave == 0) && (lane & 12) == 0) {
        const int i = lane >> 4, j = lane & 3, blk = vstart + e;
        // waves 0, 1: (cotangent row 48 + i, input row 4 blk + j); waves 2, 3 transposed: (input row 48 + i, cotangent row 4 blk + j)
        const int row = wave < 2 ? 48 + i : 4 * blk + j, c = wave < 2 ? 4 * blk + j : 48 + i;
        if (row < W) {
          if (c < W) slab[o.Vh + row * W + c] = s_;
          else if (c == W) slab[o.Vhb + row] = s_;
        }
      }
    }
  } else {
    // wave (wi, wj) owns row tiles TW wi .. x column tiles TW wj .. of dVh
#pragma unroll
    for (int t4 = 0; t4 < TW * TW; ++t4) {
      const int c = 16 * (TW * wj + (t4 % TW)) + n;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * (TW * wi + (t4 / TW)) + g + 4 * r;
        if (row < W) {
          if (c < W) slab[o.Vh + row * W + c] = accH[t4][r];
          else if (c == W) slab[o.Vhb + row] = accH[t4][r];
        }
      }
    }
  }
  __syncthreads();
  const int tid = threadIdx.x;
  if (!D::BIASROW) {   // dVh.b: the waves' sums over their points, [4 waves][16 MT rows] in the idle tile area
    double* sBsum = lds + S::oD;
#pragma unroll
    for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double s_ = xw_sum_over_n(accB[mt][r]);
        if (n == 0) sBsum[wave * 16 * D::MT + 16 * mt + 4 * r + g] = s_;
      }
    __syncthreads();
    if (tid < W) slab[o.Vhb + tid] = sBsum[tid] + sBsum[16 * D::MT + tid] + sBsum[32 * D::MT + tid] + sBsum[48 * D::MT + tid];
  }
  if (tid <= W) {
    double s_ = 0.0;
    if (tid < W) {
      const int mt = tid >> 4, gg = tid & 3, r = (tid & 15) >> 2;
      for (int wv = 0; wv < 4; ++wv) s_ += sO[(mt * 4 + r) * 16 + wv * 4 + gg];
      slab[o.Vo + tid] = s_;
    } else {
      for (int wv = 0; wv < 4; ++wv) s_ += sO[S::NO * 16 + wv * 4];
      slab[o.Vob] = s_;
    }
  }
#ifdef XW_REC_PROBE
  if (lane == 0 && blockIdx.x * 4 + wave < 2048) {
    unsigned long long* o_ = xw_rec_clock + 12 * (blockIdx.x * 4 + wave);
    for (int i = 0; i < 8; ++i) o_[i] = phc[i];
    const unsigned long long ck_out = __builtin_amdgcn_s_memtime();
    o_[8] = ck_loop - ck_in - (phc[0] + phc[1] + phc[2] + phc[3] + phc[4] + phc[5] + phc[6] + phc[7]);   // prologue
    o_[9] = ck_out - ck_loop;                                                                          // epilogue
    o_[10] = ck_out - ck_in;
    o_[11] = __builtin_amdgcn_s_memrealtime() - rt_in;
  }
#endif
}

// the compiled set: one row per container width, [NG - 1][TSUM]; from the record the depth is a run-time argument (Q = 0: the
// layer loop is rolled -- unrolled for q = 9 it spilled and was 2 % slower)
typedef void (*RecKernel)(const double*, const double*, const double*, const double*, const double*, int, int, int, double*,
                          const double*, int);
struct RecRow {
  int W;
  RecKernel k[3][2];
};
template <int W> constexpr RecRow rec_row() {
  return {W, {{k_disc_rec<W, 0, 1, false>, k_disc_rec<W, 0, 1, true>},
              {k_disc_rec<W, 0, 2, false>, k_disc_rec<W, 0, 2, true>},
              {k_disc_rec<W, 0, 3, false>, k_disc_rec<W, 0, 3, true>}}};
}
const RecRow rec_table[] = {rec_row<50>(), rec_row<64>(), rec_row<96>(), rec_row<128>()};

}  // namespace

int xw_disc_rec_launch(int W, int ng, bool tsum, int blocks, const double* xT, const double* t, const double* tpp,
                       const double* phi, const double* vbar, int N, int L, int d, double* gslab, const double* act, int q,
                       void* stream) {
  if (ng < 1 || ng > 3) return XW_E_DIMS;
  for (const RecRow& row : rec_table)
    if (row.W == W) {
      hipLaunchKernelGGL(row.k[ng - 1][tsum ? 1 : 0], dim3(blocks), dim3(256), 0, (hipStream_t)stream, xT, t, tpp, phi, vbar, N, L,
                         d, gslab, act, q);
      return xw_launch_status();
    }
  return XW_E_DIMS;
}

#ifdef XW_REC_PROBE
extern "C" int xw_debug_rec_clock(unsigned long long* host, int nwaves) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(xw_rec_clock), sizeof(unsigned long long) * 12 * nwaves);
}
#endif
