// xw_disc_fwd.hip -- adversarial test network v_phi on gfx950: the forward kernel k_disc_fwd (all 48 instantiations) with its
// ticket queue, the x-projection k_disc_xproj and their entry points.  xw_disc_core.h has the overview of the family.
#include "xw_disc_core.h"
#include <atomic>

namespace {

// ------------------------------------------------------------------------------------------------------------------
#define XW_VIN_KS 6  // k-steps of the input layer (d <= 24) whose A-fragments k_disc_fwd keeps in LDS (44 KB per block in all:
#define XW_VIN_KS_WIDE 13  // second instantiation: d <= 52 entirely from LDS (57 KB per block), wider inputs (d = 100: 25 k-steps)
                           // take their first 13 k-steps from LDS and the rest from global memory
                     // two of its blocks and two blocks of the duo sweep still share a CU's 160 KB)

// DYN: only a wave's first tile is its static one; every later tile comes from ticket counters (one returning atomic per
// tile by lane 0, issued before the input layer and read after it).  A SIMD's vector and FP64 matrix instructions add up
// across all waves it hosts (profiles/r02_probe_coexec.txt), and with 3/4 of the block slots every second CU hosts two
// blocks of this kernel and the others one block plus the stepper's waves: a static split ends with the most loaded SIMD.
// The waves of a launch move in step, so their fetches come in bursts and one word serves only ~88 atomics/us: the tiles
// after the first round are dealt round-robin to XW_DISC_NQ sub-queues (one 256-byte line each), a block's home queue is
// blockIdx mod NQ, and a wave whose queue ran dry tries the next XW_DISC_STEAL ones before it stops.  The last wave out
// (LDS count per block, then one global count) zeroes the words for the slot's next launch.
#define XW_DISC_NQ 32
#define XW_DISC_STEAL 3
#define XW_DISC_QSTRIDE 64
#define XW_DISC_SLOTS 128
__device__ unsigned int xw_disc_queue[XW_DISC_SLOTS][(XW_DISC_NQ + 1) * XW_DISC_QSTRIDE];
#ifdef XW_CLOCK_PROBE   // diagnostic build only (tools/probe_disc_clock.py): shader clocks / 100 MHz ticks of every wave's tile loop
__device__ unsigned long long xw_clock_buf[2 * 4096];
#endif
#ifndef XW_DISC_FWD_WAVES
#define XW_DISC_FWD_WAVES 2     // waves per SIMD the register allocation leaves room for (2: 256 registers, 3: 168)
#endif
// VKS: k-steps of the input layer kept in LDS (0: none; -1: the x-projection Vin[:, 1..d] x + Vin.b of every PATH is handed in,
// `xproj`, and the input layer of a point is one load and one multiply-add per row: on vertical paths the d columns of the input
// layer do not move along a path -- L = 32..64 times the same d W multiply-adds per path, 12 % of the launch's matrix
// instructions at d = 100 and 25 + 48 loads per tile)
template <int W, bool ACT, bool DYN, int VKS>
__global__ void __launch_bounds__(256, (W > 64 ? 1 : XW_DISC_FWD_WAVES)) k_disc_fwd(const double* __restrict__ xT, const double* __restrict__ tf,
                                                     const double* __restrict__ tpp, const double* __restrict__ ph, int N,
                                                     int L, int d, int q, double* __restrict__ v, double* __restrict__ vt,
                                                     double* __restrict__ gxv, double* __restrict__ gtv, int ngrad,
                                                     double* __restrict__ act, unsigned int* __restrict__ queue,
                                                     const double* __restrict__ xproj) {
  typedef VDim<W> D;
  // Vh as MFMA A-fragments in LDS (26.6 KB), shared by the 4 waves of the block: one ds_read_b64 feeds two 64-cycle MFMAs
  // (value and d/dt tangent), and keeping them out of the register file lets two waves share a SIMD so that one wave's
  // relu / tanh VALU work overlaps the other's matrix work.
  __shared__ double sVh[D::MTF * D::KS * 64];
  __shared__ double sB[2 * 16 * D::MT];
  __shared__ double sT[D::KS * 4 * (D::VTAIL ? D::TR : 1)];   // Vh[16 (MT-1) + r][4 ks + g]: the tail rows, per lane group
  __shared__ unsigned int sMask[XW_QMAX][256];     // ReLU masks (4 MT rows per lane) of the layers, for the fused reverse chain
  // input layer: Vin[:, 1..d] as A-fragments, Vin[:, 0] and Vin.b as row vectors.  From global memory they were 52 loads per
  // tile (the fragment loads put the four lanes of a quad into four rows) and their address arithmetic, re-formed for
  // every tile to keep them out of the spilled loop-invariant set
  constexpr bool VINLDS = VKS > 0;
  constexpr bool XPROJ = VKS < 0;
  __shared__ double sVin[VINLDS ? VKS * D::MT * 64 : 1];
  __shared__ double sIn[(VINLDS || XPROJ) ? 2 * 16 * D::MT : 1];
  __shared__ unsigned int sDone;
  if (DYN && threadIdx.x == 0) sDone = 0;
  // (s_setprio for this kernel's waves: no gain at 1, -5 % at 3 -- the sub-step's SIMD time is conserved)
  const int lane = xw_lane(), g = lane >> 4;
  const int wave = threadIdx.x >> 6;
  const VOff o = v_offsets(d, W);
  const long P = (long)N * L;
  const long ntiles = (P + 15) / 16;
  // (Vh.b through the padding column W of the k-range, so that a layer's accumulators start from the inline constant zero
  //  instead of 12 bias registers read from LDS: built, same time -- LDS reads do not cost the SIMD's issue cycles)
  for (int idx = wave; idx < D::MTF * D::KS; idx += 4) {
    const int mt = idx / D::KS, ks = idx - mt * D::KS;
    sVh[idx * 64 + lane] = xw_fragA(ph + o.Vh, W, W, W, 16 * mt, 4 * ks);
  }
  if (threadIdx.x < 16 * D::MT) {
    sB[threadIdx.x] = (int)threadIdx.x < W ? ph[o.Vhb + threadIdx.x] : 0.0;
    sB[16 * D::MT + threadIdx.x] = (int)threadIdx.x < W ? ph[o.Vo + threadIdx.x] : 0.0;
    if (VINLDS || XPROJ) {
      sIn[threadIdx.x] = (int)threadIdx.x < W ? ph[o.Vin + (long)threadIdx.x * o.ldin] : 0.0;
      sIn[16 * D::MT + threadIdx.x] = (int)threadIdx.x < W ? ph[o.Vinb + threadIdx.x] : 0.0;
    }
  }
  const int ksd = (d + 3) / 4;
  const int ksl = ksd < VKS ? ksd : VKS;                       // k-steps served from LDS; ksl .. ksd - 1 from global memory
  if (VINLDS)
    for (int idx = wave; idx < ksl * D::MT; idx += 4) {
      const int ks = idx / D::MT, mt = idx - ks * D::MT;
      sVin[idx * 64 + lane] = xw_fragA(ph + o.Vin + 1, o.ldin, W, d, 16 * mt, 4 * ks);
    }
  if (D::VTAIL)
    for (int idx = threadIdx.x; idx < D::KS * 4 * D::TR; idx += blockDim.x) {
      const int r = idx % D::TR, k = idx / D::TR;                        // k = 4 ks + g
      sT[idx] = k < W ? ph[o.Vh + (long)(16 * (D::MT - 1) + r) * W + k] : 0.0;
    }
  __syncthreads();
  // (starting the two waves of a SIMD -- different blocks, launched together -- out of phase by part of a layer changes nothing:
  //  220.4 / 222.0 / 221.5 us at 0 / 2048 / 4096 clocks of offset, profiles/r06_disc_fwd_stagger.txt; a lone wave per SIMD already
  //  reaches 91 % of the two-wave rate)
  const double vob = ph[o.Vob];
  // Static split: wave gw takes tiles gw, gw + G, ... (G waves in the grid), so ntiles mod G waves carry one tile more
  // than the others.  The tiles of the first time index also run the fused reverse chain (about one more tile's worth of
  // work): the first round is rotated so that THEY land on waves with the smaller count -- the launch ends with the
  // slowest wave, 6 tile-times instead of 7 at the headline size (5.33 tiles per wave).
  const long G = (long)gridDim.x * 4;
  const long rot = ntiles >= G ? ntiles % G : 0;
  // (wave-uniform) sub-queues of this launch -- every one has a home block, which only stops once it is dry --, the one in
  // use, dry queues seen
  const int nq = (int)gridDim.x < XW_DISC_NQ ? (int)gridDim.x : XW_DISC_NQ;
  int cur = blockIdx.x % nq, tries = 0;
  int zr = 0;                                // zero, opaque to the compiler (see the layer's relu / gate)
  asm volatile("" : "+v"(zr));
#ifdef XW_CLOCK_PROBE
  const unsigned long long ck0 = __builtin_amdgcn_s_memtime(), rt0 = __builtin_amdgcn_s_memrealtime();
#endif
  for (long it = (long)blockIdx.x * 4 + wave; it < ntiles;) {
    const long tile = DYN ? it : (it < G ? it - rot + (it < rot ? G : 0) : it);
    long nxt = it + G;
    unsigned int ticket = 0;
    if (DYN && lane == 0) ticket = atomicAdd(queue + cur * XW_DISC_QSTRIDE, 1u);
    const Pt pt = locate(tile, P, N, tf, tpp);
    // nabla phi is only read at the first time index: the leading `ngrad` points (time-major
    // order) also get the input gradient of v, by a reverse chain through the masks stashed below
    const bool want_grad = gxv != nullptr && tile * 16 < ngrad;         // wave-uniform
    d4 a[D::MT], ad[D::MT];
    // The record is TILE-MAJOR: [tile of 16 points][(q+1) W rows][16] -- the 4 rows x 16 points a store instruction
    // covers are 512 contiguous bytes, and everything a wave writes (or k_disc_rec reads) for one tile is one 64 KB
    // stretch (row-major, the same accesses were 128-byte pieces 1 MB apart).  Every lane of the last tile has a slot.
    const long tu = __builtin_amdgcn_readfirstlane((int)tile);          // wave-uniform by construction: a scalar base
    double* actl = act + tu * ((long)(q + 1) * W * 16);                 // (laundered like pht below: the row addresses
    asm volatile("" : "+s"(actl));                                      //  are formed per tile, not hoisted)
    const int aoff = lane;                                              // (g, n) -> row offset g, point n
    const double* pht = ph;                                             // laundered: keeps the input-layer fragment
    asm volatile("" : "+s"(pht));                                       // addresses out of the loop-invariant (spilled) set
    if (XPROJ) {
      // input layer from the path's x-projection (rows >= W of it are zero): a_0 = (Vin[:, 1..d] x + Vin.b) + Vin[:, 0] t
      // (the row offsets (16 mt + 4 r + g) N do not change from tile to tile: formed HERE, from a copy of N the compiler cannot see
      //  through -- hoisted out of the tile loop they stay live across the layers and go to scratch, like the fragment addresses above)
      int Nl = N;
      asm volatile("" : "+s"(Nl));
      const double* xp = xproj + pt.n + (long)g * Nl;
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ad[mt][r] = sIn[16 * mt + g + 4 * r];
          a[mt][r] = (16 * mt + 4 * r < W) ? fma(ad[mt][r], pt.t, xw_ld_g(xp + (long)(16 * mt + 4 * r) * Nl)) : 0.0;
        }
    } else if (VINLDS) {
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ad[mt][r] = sIn[16 * mt + g + 4 * r];
          a[mt][r] = sIn[16 * D::MT + 16 * mt + g + 4 * r] + ad[mt][r] * pt.t;
        }
      for (int ks = 0; ks < ksl; ++ks) {
        const int i = 4 * ks + g;
        const double b = i < d ? xT[(long)i * N + pt.n] : 0.0;
#pragma unroll
        for (int mt = 0; mt < D::MT; ++mt) a[mt] = XW_MFMA(sVin[(ks * D::MT + mt) * 64 + lane], b, a[mt]);
      }
      for (int ks = ksl; ks < ksd; ++ks) {                             // (d > 4 VKS: the rest of the input rows)
        const int i = 4 * ks + g;
        const double b = i < d ? xT[(long)i * N + pt.n] : 0.0;
#pragma unroll
        for (int mt = 0; mt < D::MT; ++mt) a[mt] = XW_MFMA(xw_fragA(pht + o.Vin + 1, o.ldin, W, d, 16 * mt, 4 * ks), b, a[mt]);
      }
    } else {
      input_layer<W>(pht, o, xT, N, d, pt, a, ad);
    }
    // relu'(+0) = 0 (torch): the layers below gate the d/dt tangent by the SIGN bit of the pre-activation, which is open at an
    // exact +0.  In a tied layer an exact +0 is a unit whose inputs are all dead -- its tangent is a sum of gated zeros -- but
    // HERE it can come from the input itself (t = 0, x = 0 with the zero bias the network starts from) with a tangent Vin[:, 0]
    // that is not zero: an exact zero leaves the input layer as -0, which every later test treats as "closed" (once per tile,
    // 2 vector instructions per register).
#pragma unroll
    for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double x = a[mt][r];
        a[mt][r] = __hiloint2double(x == 0.0 ? (int)0x80000000 : __double2hiint(x), __double2loint(x));
      }
    if (DYN) {
      nxt = G + cur + (long)nq * (unsigned int)__builtin_amdgcn_readfirstlane((int)ticket);
      while (nxt >= ntiles && tries < XW_DISC_STEAL && tries + 1 < nq) {      // home queue dry: the neighbours' (rare, end of the launch)
        ++tries;
        cur = cur + 1 < nq ? cur + 1 : 0;
        if (lane == 0) ticket = atomicAdd(queue + cur * XW_DISC_QSTRIDE, 1u);
        nxt = G + cur + (long)nq * (unsigned int)__builtin_amdgcn_readfirstlane((int)ticket);
      }
    }
    // one tied layer (value and d/dt tangent): (ai, adi) -> (nw, nd).  The loop below alternates two register sets so
    // that no layer ends with 32 register moves (a wave's VALU work does not overlap its FP64 MFMAs).
    auto layer = [&](int j, const d4 (&ai)[D::MT], const d4 (&adi)[D::MT], d4 (&nw)[D::MT], d4 (&nd)[D::MT]) {
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) nw[mt][r] = sB[16 * mt + g + 4 * r];
        nd[mt] = xw_zero4();
      }
      if (want_grad) {                                      // (wave-uniform; 1 tile in L needs the masks)
        unsigned int mask = 0;
#pragma unroll
        for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) mask |= (ai[mt][r] > 0.0 ? 1u : 0u) << (4 * mt + r);
        sMask[j][threadIdx.x] = mask;
      }
      double tv[D::TR], td[D::TR];                          // partial dot products of the tail rows (this lane's k = 4 ks + g)
#pragma unroll
      for (int r = 0; r < D::TR; ++r) tv[r] = td[r] = 0.0;
      // A-fragments (and the tail rows' weights) of k-step ks + 1 are requested from LDS BEFORE the matrix instructions of
      // k-step ks: a wave alone on its SIMD (640 of the 1024 SIMDs as launched beside the stepper) otherwise stops at a
      // wait in front of almost every pair of MFMAs
      double wn[D::MTF], tn[D::TR];
#pragma unroll
      for (int mt = 0; mt < D::MTF; ++mt) wn[mt] = sVh[(mt * D::KS) * 64 + lane];
      if (D::VTAIL)
#pragma unroll
        for (int r = 0; r < D::TR; ++r) tn[r] = sT[g * D::TR + r];
#pragma unroll
      for (int ks = 0; ks < D::KS; ++ks) {
        const double av = ai[ks >> 2][ks & 3];
        // relu and the tangent's gate from ONE 32-bit word, the sign extension of av's high word: x & ~sgn as a single
        // v_bfi_b32 per 32-bit half (sgn ? zr : x, zr a register that holds zero but is opaque to the compiler -- with a
        // visible zero, or a visible sign test, it rewrites the bit operations into compare + v_cndmask_b32 again).
        // 1 + 4 instructions of 2.3 clocks per k-step where v_max_f64 x 2 (canonicalise + max), v_or, v_mov, v_cmp_ne_u64 and
        // two v_cndmask_b32 took ~31.  av >= +0 keeps both, av < 0 (or -0) clears both: at av == +0 exactly the gate stays
        // open where torch's relu' is 0 -- in a tied layer that only happens where the tangent is zero as well (padding units,
        // dead inputs); the input layer's exact zeros arrive here as -0 (above).
        int sgn = __double2hiint(av) >> 31;
        asm volatile("" : "+v"(sgn));
        const double adv = adi[ks >> 2][ks & 3];
        const double b = __hiloint2double((sgn & zr) | (~sgn & __double2hiint(av)), (sgn & zr) | (~sgn & __double2loint(av)));
        const double bd = __hiloint2double((sgn & zr) | (~sgn & __double2hiint(adv)), (sgn & zr) | (~sgn & __double2loint(adv)));
        if (ACT) {   // activation store: row j W + k of the record is the layer input relu(a_j)[k], point-major
          double* __restrict__ rowp = actl + (j * W + 4 * ks) * 16;             // uniform pointer + 32-bit lane offset
          if (4 * ks + 3 < W || 4 * ks + g < W) xw_st_nt(b, rowp + aoff);   // (streamed: read once, much later)
        }
        double wc[D::MTF], tc[D::TR];
#pragma unroll
        for (int mt = 0; mt < D::MTF; ++mt) wc[mt] = wn[mt];
#pragma unroll
        for (int r = 0; r < D::TR; ++r) tc[r] = D::VTAIL ? tn[r] : 0.0;
        if (ks + 1 < D::KS) {
#pragma unroll
          for (int mt = 0; mt < D::MTF; ++mt) wn[mt] = sVh[(mt * D::KS + ks + 1) * 64 + lane];
          if (D::VTAIL)
#pragma unroll
            for (int r = 0; r < D::TR; ++r) tn[r] = sT[(4 * (ks + 1) + g) * D::TR + r];
        }
        asm volatile("" ::: "memory");                      // the requests stay HERE, one k-step ahead of their use
#pragma unroll
        for (int mt = 0; mt < D::MTF; ++mt) {
          nw[mt] = XW_MFMA(wc[mt], b, nw[mt]);
          nd[mt] = XW_MFMA(wc[mt], bd, nd[mt]);
        }
        if (D::VTAIL) {
#pragma unroll
          for (int r = 0; r < D::TR; ++r) {
            tv[r] = fma(tc[r], b, tv[r]);
            td[r] = fma(tc[r], bd, td[r]);
          }
        }
      }
      if (D::VTAIL && D::TR == 2) {
        // the four partials (value / tangent of rows 48, 49) -> ONE register with the totals in the four lane groups
        // (g = 0: row 48, g = 1: row 49, g = 2, 3: the two tangent totals), then the tangent's copy with the halves swapped.
        // Rows 50, 51 of both tiles (lane groups 2, 3) then hold finite leftovers instead of zeros: they only ever meet
        // zero-padded weights (columns >= W of the Vh fragments and of the tail rows, rows >= W of Vo and of Vh^T), and the
        // record's stores are guarded by row < W.  8 swaps + 4 adds where four separate sums took 16 + 8 and 8 selects.
        const double R = xw_fold16(xw_fold32(tv[0], td[0]), xw_fold32(tv[1], td[1]));
        d4 tw = xw_zero4(), tdd = xw_zero4();
        tw[0] = R + nw[D::MT - 1][0];
        const unsigned rl = __double2loint(R), rh = __double2hiint(R);
        typedef unsigned xw_u2 __attribute__((ext_vector_type(2)));
        const xw_u2 sl = __builtin_amdgcn_permlane32_swap(rl, rl, false, false), sh = __builtin_amdgcn_permlane32_swap(rh, rh, false, false);
        tdd[0] = __hiloint2double(sh[1], sl[1]);              // (R[32..63], R[32..63]): tangent totals in lane groups 0, 1
        nw[D::MT - 1] = tw;
        nd[D::MT - 1] = tdd;
      } else
      if (D::VTAIL) {   // row 16 (MT-1) + r of the chain layout lives in lane group g = r, register 0
        d4 tw = xw_zero4(), tdd = xw_zero4();
#pragma unroll
        for (int r = 0; r < D::TR; ++r) {
          const double sv_ = xw_sum_over_g(tv[r]) + nw[D::MT - 1][0], sd_ = xw_sum_over_g(td[r]);
          if (g == r) {
            tw[0] = sv_;
            tdd[0] = sd_;
          }
        }
        nw[D::MT - 1] = tw;
        nd[D::MT - 1] = tdd;
      }
    };
    {
      d4 b0[D::MT], bd0[D::MT];
      int j = 0;
      for (; j + 1 < q; j += 2) {
        layer(j, a, ad, b0, bd0);
        layer(j + 1, b0, bd0, a, ad);
      }
      if (j < q) {
        layer(j, a, ad, b0, bd0);
#pragma unroll
        for (int mt = 0; mt < D::MT; ++mt) {
          a[mt] = b0[mt];
          ad[mt] = bd0[mt];
        }
      }
    }
    double sv = 0.0, sd = 0.0;
#pragma unroll
    for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (16 * mt + 4 * r < W) {  // rows 16 mt + 4 r + g >= W only carry zero padding
          const double th = xw_tanh(a[mt][r]);
          if (ACT && (16 * mt + 4 * r + 3 < W || 16 * mt + 4 * r + g < W))
            xw_st_nt(th, actl + (q * W + 16 * mt + 4 * r) * 16 + aoff);   // last rows: tanh(a_q)
          const double vo = sB[16 * D::MT + 16 * mt + g + 4 * r];
          sv += vo * th;
          sd += vo * (1.0 - th * th) * ad[mt][r];
          a[mt][r] = vo * (1.0 - th * th);       // reused below as the cotangent of a_q for d(sum v)/d(input)
        } else {
          a[mt][r] = 0.0;
        }
    sv = xw_sum_over_g(sv) + vob;
    sd = xw_sum_over_g(sd);
    if (g == 0 && pt.valid) {
      v[pt.p] = sv;
      if (vt != nullptr) vt[pt.p] = sd;
    }
    if (want_grad) {
      // reverse chain: delta_j = relu'(a_j) .* (Vh^T delta_{j+1}); Vh^T fragments come from L2 (1 tile in L is affected).
      // The base pointer is laundered so that the per-lane fragment addresses are formed HERE: hoisted out of the tile
      // loop they spilled to scratch in every wave's prologue (17 MB of scratch writes per launch in the PMC pass).
      const double* phg = ph;
      asm volatile("" : "+s"(phg));
      int ll = lane;                         // (the lane-offset part of those addresses is loop-invariant too: a copy of the
      asm volatile("" : "+v"(ll));           //  lane id the compiler cannot see through keeps it here as well)
      d4 (&dl)[D::MT] = a;
      // (Gathering the A-fragments of Vh^T from the forward fragments in LDS -- element Vh[r][c] sits in fragment (r >> 4, c >> 2)
      //  at lane (r & 15) + 16 (c & 3), so a fragment of the transpose is one ds_read with an immediate offset plus a fixed lane
      //  part -- was built and is 8-way bank-conflicted: a lone gradient tile took 36 us more than a plain one, against 42 us
      //  with the loads inside the k-step and 29 us with the L2 loads one k-step ahead as below; tools/gradtile.py.)
      auto fragT = [&](int mt, int ks) -> double { return xw_fragAT_l(phg + o.Vh, W, W, W, 16 * mt, 4 * ks, ll); };
      for (int j = q - 1; j >= 0; --j) {
        d4 nd[D::MT];
#pragma unroll
        for (int mt = 0; mt < D::MT; ++mt) nd[mt] = xw_zero4();
        // (the fragments of k-step ks + 1 are requested before the matrix instructions of k-step ks)
        double fn[D::MT];
#pragma unroll
        for (int mt = 0; mt < D::MT; ++mt) fn[mt] = fragT(mt, 0);
#pragma unroll
        for (int ks = 0; ks < D::KS; ++ks) {
          const double b = dl[ks >> 2][ks & 3];
          double fc[D::MT];
#pragma unroll
          for (int mt = 0; mt < D::MT; ++mt) fc[mt] = fn[mt];
          if (ks + 1 < D::KS) {
#pragma unroll
            for (int mt = 0; mt < D::MT; ++mt) fn[mt] = fragT(mt, ks + 1);
          }
          asm volatile("" ::: "memory");   // a few loads in flight, not all 52 (register pressure)
#pragma unroll
          for (int mt = 0; mt < D::MT; ++mt) nd[mt] = XW_MFMA(fc[mt], b, nd[mt]);
        }
        const unsigned int mask = sMask[j][threadIdx.x];
#pragma unroll
        for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) dl[mt][r] = ((mask >> (4 * mt + r)) & 1u) ? nd[mt][r] : 0.0;
      }
      int ngl = ngrad;                       // laundered: keeps the (lane-dependent) row offsets i * ngrad of the gxv stores
      asm volatile("" : "+s"(ngl));          // out of the loop-invariant set (they were spilled in every wave's prologue)
      const bool gl = pt.valid && pt.p < ngl;
      for (int rt = 0; rt < (d + 15) / 16; ++rt) {
        d4 vv = xw_zero4();
#pragma unroll
        for (int ks = 0; ks < D::KS; ++ks) {
          if ((ks & 3) == 0) asm volatile("" ::: "memory");
          vv = XW_MFMA(xw_fragAT_l(phg + o.Vin + 1, o.ldin, W, d, 16 * rt, 4 * ks, ll), dl[ks >> 2][ks & 3], vv);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * rt + g + 4 * r;
          if (i < d && gl) gxv[(long)i * ngl + pt.p] = vv[r];
        }
      }
      double st_ = 0.0;
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt) {
        const d4 v0 = xw_vecD_strided(phg + o.Vin, o.ldin, W, 16 * mt);
#pragma unroll
        for (int r = 0; r < 4; ++r) st_ += v0[r] * dl[mt][r];
      }
      st_ = xw_sum_over_g(st_);
      if (gtv != nullptr && g == 0 && gl) gtv[pt.p] = st_;
    }
    it = nxt;
  }
#ifdef XW_CLOCK_PROBE
  if (lane == 0 && blockIdx.x * 4 + wave < 4096) {
    xw_clock_buf[2 * (blockIdx.x * 4 + wave)] = __builtin_amdgcn_s_memtime() - ck0;
    xw_clock_buf[2 * (blockIdx.x * 4 + wave) + 1] = __builtin_amdgcn_s_memrealtime() - rt0;
  }
#endif
  if (DYN && lane == 0) {
    if (atomicAdd(&sDone, 1u) == 3u && atomicAdd(queue + XW_DISC_NQ * XW_DISC_QSTRIDE, 1u) == gridDim.x - 1u)
      for (int s_ = 0; s_ <= XW_DISC_NQ; ++s_) atomicExch(queue + s_ * XW_DISC_QSTRIDE, 0u);
  }
}

}  // namespace
extern "C" int xw_disc_act_rows(int W, int q) { return ((disc_width_ok(W) && q >= 0) || xwg_disc_ok(1, W, q)) ? (q + 1) * W : XW_E_DIMS; }

// x-projection of the input layer for the N paths of a group: xproj[r][n] = Vin[r, 1..d] x_n + Vin.b[r] for r < W, zero for the
// padding rows up to 64.  One thread per (path, four rows); 41 MFLOP at d = 100, N = 8192: a few microseconds.
namespace {
__global__ void __launch_bounds__(256) k_disc_xproj(const double* __restrict__ xT, const double* __restrict__ ph, int N, int d, int W,
                                                     double* __restrict__ xproj) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  const int r0 = blockIdx.y * 4;
  if (n >= N) return;
  const VOff o = v_offsets(d, W);
  const int r1 = r0 + 1 < W ? r0 + 1 : W - 1, r2 = r0 + 2 < W ? r0 + 2 : W - 1, r3 = r0 + 3 < W ? r0 + 3 : W - 1, rr = r0 < W ? r0 : W - 1;
  const double* w0 = ph + o.Vin + (long)rr * o.ldin + 1;
  const double* w1 = ph + o.Vin + (long)r1 * o.ldin + 1;
  const double* w2 = ph + o.Vin + (long)r2 * o.ldin + 1;
  const double* w3 = ph + o.Vin + (long)r3 * o.ldin + 1;
  double a0 = ph[o.Vinb + rr], a1 = ph[o.Vinb + r1], a2 = ph[o.Vinb + r2], a3 = ph[o.Vinb + r3];
#pragma unroll 4
  for (int i = 0; i < d; ++i) {
    const double x = xT[(long)i * N + n];
    a0 = fma(w0[i], x, a0);
    a1 = fma(w1[i], x, a1);
    a2 = fma(w2[i], x, a2);
    a3 = fma(w3[i], x, a3);
  }
  xproj[(long)r0 * N + n] = r0 < W ? a0 : 0.0;
  xproj[(long)(r0 + 1) * N + n] = r0 + 1 < W ? a1 : 0.0;
  xproj[(long)(r0 + 2) * N + n] = r0 + 2 < W ? a2 : 0.0;
  xproj[(long)(r0 + 3) * N + n] = r0 + 3 < W ? a3 : 0.0;
}

// the compiled set of k_disc_fwd: one row per (width, input-layer plan VKS), [ACT][DYN].  Widths 50 and 64 have all four plans;
// at 96 and 128 the fragments of Vh are 74 / 131 KB of LDS and leave none for input-layer fragments -- the x-projection
// table, or global loads.
typedef void (*FwdKernel)(const double*, const double*, const double*, const double*, int, int, int, int, double*, double*,
                          double*, double*, int, double*, unsigned int*, const double*);
struct FwdRow {
  int W, vks;
  FwdKernel k[2][2];
};
template <int W, int VKS> constexpr FwdRow fwd_row() {
  return {W, VKS, {{k_disc_fwd<W, false, false, VKS>, k_disc_fwd<W, false, true, VKS>},
                   {k_disc_fwd<W, true, false, VKS>, k_disc_fwd<W, true, true, VKS>}}};
}
const FwdRow fwd_table[] = {
    fwd_row<50, -1>(), fwd_row<50, 0>(), fwd_row<50, XW_VIN_KS>(), fwd_row<50, XW_VIN_KS_WIDE>(),
    fwd_row<64, -1>(), fwd_row<64, 0>(), fwd_row<64, XW_VIN_KS>(), fwd_row<64, XW_VIN_KS_WIDE>(),
    fwd_row<96, -1>(), fwd_row<96, 0>(), fwd_row<128, -1>(), fwd_row<128, 0>()};

// the k_disc_fwd of a call and its grid, from the shape and the switches alone (W one of the compiled widths)
struct FwdKey {
  int vks;
  bool dyn;
  long blocks;
};
FwdKey fwd_select(int W, long ntiles, int d, int max_blocks, bool xproj, bool dyn_on, bool vin_on) {
  FwdKey k;
  k.blocks = (ntiles + 3) / 4;
  const long cap = max_blocks > 0 ? max_blocks : 512;   // default: 2 blocks per CU resident (launch bounds), grid-stride over tiles
  if (k.blocks > cap) k.blocks = cap;
  // more than one round of tiles per wave: tickets (see k_disc_fwd)
  k.dyn = dyn_on && ntiles > 4 * k.blocks;
  if (W > 64) {
    // 96, 128: one block per CU (a wave holds up to 512 registers)
    if (k.blocks > 256) k.blocks = 256;
    k.dyn = k.dyn && ntiles > 4 * k.blocks;              // (the test again at the smaller grid: it can only confirm the first)
  }
  k.vks = xproj ? -1 : (!vin_on || W > 64) ? 0 : ((d + 3) / 4 <= XW_VIN_KS ? XW_VIN_KS : XW_VIN_KS_WIDE);
  return k;
}
FwdKernel fwd_kernel(int W, int vks, bool act, bool dyn) {
  for (const FwdRow& row : fwd_table)
    if (row.W == W && row.vks == vks) return row.k[act ? 1 : 0][dyn ? 1 : 0];
  return nullptr;
}
}  // namespace

extern "C" int xw_disc_xproj(const double* xT, const double* phi, int N, int d, int W, double* xproj, void* stream) {
  if (!xT || !phi || !xproj || N <= 0 || d <= 0) return XW_E_ARG;
  if (!disc_width_ok(W)) return XW_E_DIMS;
  // (the table has 16 MT rows: 64 for the widths 50 and 64, 96 / 128 for the wide containers; four rows per thread)
  hipLaunchKernelGGL(k_disc_xproj, dim3((N + 255) / 256, W > 96 ? 32 : W > 64 ? 24 : 16), dim3(256), 0, (hipStream_t)stream, xT, phi, N, d, W, xproj);
  return xw_launch_status();
}

extern "C" int xw_disc_fwd(const double* xT, const double* t, const double* tpp, const double* phi, int N, int L, int d,
                           int W, int q, double* v, double* vt, double* gxv, double* gtv, int ngrad, int max_blocks,
                           double* act, void* stream) {
  return xw_disc_fwd_xproj(xT, t, tpp, phi, N, L, d, W, q, v, vt, gxv, gtv, ngrad, max_blocks, act, nullptr, stream);
}

extern "C" int xw_disc_fwd_xproj(const double* xT, const double* t, const double* tpp, const double* phi, int N, int L, int d,
                                 int W, int q, double* v, double* vt, double* gxv, double* gtv, int ngrad, int max_blocks,
                                 double* act, const double* xproj, void* stream) {
  if (!xT || !phi || !v || N <= 0 || L <= 0 || d <= 0 || q < 0) return XW_E_ARG;
  if (!tpp && !t) return XW_E_ARG;
  if (tpp && L != 1) return XW_E_ARG;
  if (gxv && (ngrad <= 0 || (long)ngrad > (long)N * L || q > XW_QMAX)) return XW_E_ARG;
  if (!disc_width_ok(W)) return xwg_disc_fwd(xT, t, tpp, phi, N, L, d, W, q, v, vt, gxv, gtv, ngrad, act, stream);
  if (xproj != nullptr && tpp != nullptr) return XW_E_ARG;             // (point mode: every point has its own x)
  if ((long)N * L * 4 >= (1L << 31)) return XW_E_ARG;                  // 32-bit lane offsets into the activation record
  static unsigned int* qbase = [] { void* p = nullptr; (void)hipGetSymbolAddress(&p, HIP_SYMBOL(xw_disc_queue)); return (unsigned int*)p; }();
  static std::atomic<unsigned int> next_slot[2];        // [0]: eager launches, [1]: launches recorded into a graph
  const XwSwitches& sw = xw_switches();
  const FwdKey k = fwd_select(W, ((long)N * L + 15) / 16, d, max_blocks, xproj != nullptr, sw.disc_dynamic != 0 && qbase != nullptr,
                              sw.disc_vin_lds != 0);
  // every ticketed launch takes the next queue slot: launches that can overlap in time never share one
  unsigned int* queue = nullptr;
  if (k.dyn) {
    // a captured launch keeps its slot for every replay: the two kinds draw from separate halves of the slot array, so
    // that an eager launch (module calls between sub-steps, other streams) can never meet a replay on the same words
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) cs = hipStreamCaptureStatusNone;
    const int half = cs == hipStreamCaptureStatusActive ? 1 : 0;
    const unsigned int slot = half * (XW_DISC_SLOTS / 2) + next_slot[half].fetch_add(1) % (XW_DISC_SLOTS / 2);
    queue = qbase + (size_t)slot * ((XW_DISC_NQ + 1) * XW_DISC_QSTRIDE);
  }
  // (Two 16-point tiles per wave at one wave per SIMD -- every A-fragment read feeding four matrix instructions, 360-410 registers,
  //  no scratch, results bit-identical -- was built and measured in round 6 and LOSES: 214.9 against 201.4 us without the gradient
  //  tiles, 273.5 against 220.4 us with them (static split over pairs); profiles/r06_disc_fwd_two_tiles_per_wave.txt.  Two waves of
  //  one tile each are the better way to fill a SIMD at this width; the kernel was removed again.)
  const FwdKernel kernel = fwd_kernel(W, k.vks, act != nullptr, k.dyn);
  if (kernel == nullptr) return XW_E_DIMS;
  hipLaunchKernelGGL(kernel, dim3((unsigned)k.blocks), dim3(256), 0, (hipStream_t)stream, xT, t, tpp, phi, N, L, d, q, v, vt, gxv,
                     gtv, ngrad, act, queue, xproj);
  return xw_launch_status();
}

#ifdef XW_CLOCK_PROBE
extern "C" int xw_debug_clock(unsigned long long* host, int nwaves) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(xw_clock_buf), sizeof(unsigned long long) * 2 * nwaves);
}
#endif
