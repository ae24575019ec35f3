// xw_disc_bwd.hip -- adversarial test network v_phi on gfx950: the reverse entry points xw_disc_bwd (which chooses between the
// generic path, k_disc_rec of xw_disc_rec.hip and the recomputing kernel), xw_disc_gradx and xw_disc_bwd_slabs, and the
// recomputing reverse kernel k_disc_bwd (all 4 instantiations).  xw_disc_core.h has the overview of the family.
#include "xw_disc_core.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// LDS plan of k_disc_bwd (doubles):  Vh frags | Vh^T frags | delta T-tiles [4 waves][MT] | r T-tiles [4][MT] | dVo acc
template <int W> struct BwdLds {
  typedef VDim<W> D;
  static constexpr int nfrag = D::MT * D::KS * 64;
  static constexpr int ntt = 4 * D::MT * XW_TTILE;
  static constexpr int oVh = 0, oVhT = nfrag, oD = 2 * nfrag, oR = 2 * nfrag + ntt, oO = 2 * nfrag + 2 * ntt;
  static constexpr int oB = oO + 4 * 64 * 16;     // Vh.b and Vo, zero-padded to 16 MT rows each
  static constexpr int total = oB + 2 * 16 * D::MT;
  static_assert(total * 8 <= 160 * 1024, "LDS budget of one CU");
};

// (the parameter gradient from the activation record is k_disc_rec of xw_disc_rec.hip; this kernel recomputes the forward per tile)
template <int W, int Q, int CTG, bool PARAMS, bool INGRAD>
__global__ void __launch_bounds__(256) k_disc_bwd(const double* __restrict__ xT, const double* __restrict__ tf,
                                                  const double* __restrict__ tpp, const double* __restrict__ ph,
                                                  const double* __restrict__ vbar, int N, int L, int d,
                                                  double* __restrict__ gslab, double* __restrict__ gxv,
                                                  double* __restrict__ gtv) {
  typedef VDim<W> D;
  typedef BwdLds<W> S;
  static_assert(D::MT == 4, "the recomputing reverse kernel maps the 4 row tiles of dVh onto the 4 waves of a block");
  static_assert(D::BIASROW, "the recomputing reverse kernel takes dVh.b from the ones row");
  __shared__ double lds[S::total];
  double* sVh = lds + S::oVh;
  double* sVhT = lds + S::oVhT;
  double* sD = lds + S::oD;
  double* sR = lds + S::oR;
  double* sO = lds + S::oO;
  const int lane = xw_lane(), g = lane >> 4, n = lane & 15;
  const int wave = threadIdx.x >> 6;
  const VOff o = v_offsets(d, W);
  const long P = (long)N * L;
  const long nsuper = (P + 63) / 64;

  double* sB = lds + S::oB;
  for (int idx = wave; idx < D::MT * D::KS; idx += 4) {
    const int mt = idx / D::KS, ks = idx - mt * D::KS;
    sVh[idx * 64 + lane] = xw_fragA(ph + o.Vh, W, W, W, 16 * mt, 4 * ks);
    sVhT[idx * 64 + lane] = xw_fragAT(ph + o.Vh, W, W, W, 16 * mt, 4 * ks);
  }
  if (threadIdx.x < 16 * D::MT) {
    sB[threadIdx.x] = (int)threadIdx.x < W ? ph[o.Vhb + threadIdx.x] : 0.0;
    sB[16 * D::MT + threadIdx.x] = (int)threadIdx.x < W ? ph[o.Vo + threadIdx.x] : 0.0;
  }
  if (PARAMS)
    for (int i = 0; i < 16; ++i) sO[i * 256 + wave * 64 + lane] = 0.0;   // [slot][thread]: lane-contiguous, no bank conflicts
  __syncthreads();

  d4 accH[D::MT], accIn[CTG * 4];
#pragma unroll
  for (int ct = 0; ct < D::MT; ++ct) accH[ct] = xw_zero4();
#pragma unroll
  for (int ct = 0; ct < CTG * 4; ++ct) accIn[ct] = xw_zero4();

  // one tied hidden layer  a_out = Vh.b + Vh r  with A-fragments and the bias read from LDS
  auto layer = [&](const d4 (&r)[D::MT], d4 (&out)[D::MT]) {
    asm volatile("" ::: "memory");   // keep the A-fragments in LDS: without this the compiler hoists all 52 loads of
                                     // every unrolled layer into registers and spills the activations instead
#pragma unroll
    for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) out[mt][rr] = sB[16 * mt + g + 4 * rr];
#pragma unroll
    for (int ks = 0; ks < D::KS; ++ks) {
      const double b = r[ks >> 2][ks & 3];
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt) out[mt] = XW_MFMA(sVh[(mt * D::KS + ks) * 64 + lane], b, out[mt]);
    }
  };

  // layers per checkpoint segment.  1: every layer input r_j stays in registers (13 live f64 per layer at W = 50) and
  // nothing is recomputed -- 497 vs 558 us at SEG = 3 even with 48 spilled registers.  The wide-input variant (CTG = 2,
  // d > 62) carries 32 more accumulator registers and keeps the 3-layer segments.
  constexpr int SEG = CTG == 1 ? 1 : 3;
  constexpr int NSEG = (Q + SEG - 1) / SEG;
  for (long st = blockIdx.x; st < nsuper; st += gridDim.x) {
    const Pt pt = locate(st * 4 + wave, P, N, tf, tpp);
    // ---- forward: only r_0, r_3, r_6 (= relu(a_j)) are kept; the layers in between are recomputed per segment, so the
    //      live activations are 2 x SEG tiles instead of Q (which did not fit the 512-register file and spilled)
    d4 ck[NSEG][D::MT];
    d4 a[D::MT], ad[D::MT];
    input_layer<W>(ph, o, xT, N, d, pt, a, ad);
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      d4 r[D::MT];
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt) {
#pragma unroll
        for (int q_ = 0; q_ < 4; ++q_)
          if (q_ < D::LR(mt)) {
            r[mt][q_] = a[mt][q_] > 0.0 ? a[mt][q_] : 0.0;
            if (j % SEG == 0) ck[j / SEG][mt][q_] = r[mt][q_];
          }
      }
      layer(r, a);
    }
    // ---- output layer and its cotangent
    const double vb = pt.valid ? (vbar != nullptr ? vbar[pt.p] : 1.0) : 0.0;
    d4 dl[D::MT];
#pragma unroll
    for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double th = 0.0;
        if (16 * mt + 4 * r < W) th = xw_tanh(a[mt][r]);
        dl[mt][r] = sB[16 * D::MT + 16 * mt + g + 4 * r] * (1.0 - th * th) * vb;
        if (PARAMS) sO[(mt * 4 + r) * 256 + wave * 64 + lane] += (mt == D::MT - 1 && r == 3) ? (g == 0 ? vb : 0.0) : vb * th;
      }
    // ---- reverse chain, segment by segment
#pragma unroll
    for (int sg = NSEG - 1; sg >= 0; --sg) {
      d4 seg[SEG][D::MT];
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
        for (int q_ = 0; q_ < 4; ++q_)
          if (q_ < D::LR(mt)) seg[0][mt][q_] = ck[sg][mt][q_];
#pragma unroll
      for (int k = 1; k < SEG; ++k)
        if (sg * SEG + k < Q) {
          d4 tmp[D::MT];
          layer(seg[k - 1], tmp);
#pragma unroll
          for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
            for (int q_ = 0; q_ < 4; ++q_)
              if (q_ < D::LR(mt)) seg[k][mt][q_] = tmp[mt][q_] > 0.0 ? tmp[mt][q_] : 0.0;
        }
#pragma unroll
      for (int k = SEG - 1; k >= 0; --k) {
        if (sg * SEG + k >= Q) continue;
        if (PARAMS) {
#pragma unroll
          for (int mt = 0; mt < D::MT; ++mt) {
            d4 rj = seg[k][mt];
            if (mt == (W >> 4)) {
              if (g == ((W & 15) & 3)) rj[(W & 15) >> 2] = 1.0;  // ones row -> column W of dVh collects dVh.b
            }
            if (mt < D::MT - 1) {
              xw_writeT(sD + (wave * D::MT + mt) * XW_TTILE, dl[mt]);
              xw_writeT(sR + (wave * D::MT + mt) * XW_TTILE, rj);
            } else {
              xw_writeT_n<D::LR(D::MT - 1)>(sD + (wave * D::MT + mt) * XW_TTILE, dl[mt]);
              xw_writeT_n<D::LR(D::MT - 1)>(sR + (wave * D::MT + mt) * XW_TTILE, rj);
            }
          }
        }
        // reverse chain first: its 52 MFMAs only need dl and Vh^T and cover the latency of the LDS transposes above
        d4 nd[D::MT];
        asm volatile("" ::: "memory");
#pragma unroll
        for (int mt = 0; mt < D::MT; ++mt) nd[mt] = xw_zero4();
#pragma unroll
        for (int ks = 0; ks < D::KS; ++ks) {
          const double b = dl[ks >> 2][ks & 3];
#pragma unroll
          for (int mt = 0; mt < D::MT; ++mt) nd[mt] = XW_MFMA(sVhT[(mt * D::KS + ks) * 64 + lane], b, nd[mt]);
        }
        if (PARAMS) {
          __syncthreads();
#pragma unroll
          for (int pw = 0; pw < 4; ++pw)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
              const double av = xw_readT(sD + (pw * D::MT + wave) * XW_TTILE, ks);
#pragma unroll
              for (int ct = 0; ct < D::MT; ++ct)
                accH[ct] = XW_MFMA(av, xw_readT(sR + (pw * D::MT + ct) * XW_TTILE, ks), accH[ct]);
            }
          __syncthreads();
        }
#pragma unroll
        for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (r < D::LR(mt)) dl[mt][r] = seg[k][mt][r] > 0.0 ? nd[mt][r] : 0.0;
      }
    }
    // ---- dl = cotangent of a_0.  Input layer: dVin = dl (x) [t; x; 1]
    if (PARAMS) {
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt) xw_writeT(sD + (wave * D::MT + mt) * XW_TTILE, dl[mt]);
#pragma unroll
      for (int grp = 0; grp < CTG; ++grp) {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          const int cl = g + 4 * rr;            // local row 0..63 of this group
          const int c = 64 * grp + cl;          // input row: 0 = t, 1..d = x, d+1 = ones
          double val = 0.0;
          if (pt.valid) {
            if (c == 0) val = pt.t;
            else if (c <= d) val = xT[(long)(c - 1) * N + pt.n];
            else if (c == d + 1) val = 1.0;
          }
          sR[(wave * D::MT + (cl >> 4)) * XW_TTILE + (cl & 15) * XW_TSTRIDE + n] = val;
        }
        __syncthreads();
#pragma unroll
        for (int pw = 0; pw < 4; ++pw)
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const double av = xw_readT(sD + (pw * D::MT + wave) * XW_TTILE, ks);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
              accIn[grp * 4 + ct] = XW_MFMA(av, xw_readT(sR + (pw * D::MT + ct) * XW_TTILE, ks), accIn[grp * 4 + ct]);
          }
        __syncthreads();
      }
    }
    if (INGRAD) {
      for (int rt = 0; rt < (d + 15) / 16; ++rt) {
        d4 vv = xw_zero4();
#pragma unroll
        for (int ks = 0; ks < D::KS; ++ks)
          vv = XW_MFMA(xw_fragAT(ph + o.Vin + 1, o.ldin, W, d, 16 * rt, 4 * ks), dl[ks >> 2][ks & 3], vv);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * rt + g + 4 * r;
          if (i < d && pt.valid) gxv[(long)i * P + pt.p] = vv[r];
        }
      }
      double st_ = 0.0;
#pragma unroll
      for (int mt = 0; mt < D::MT; ++mt) {
        const d4 v0 = xw_vecD_strided(ph + o.Vin, o.ldin, W, 16 * mt);
#pragma unroll
        for (int r = 0; r < 4; ++r) st_ += v0[r] * dl[mt][r];
      }
      st_ = xw_sum_over_g(st_);
      if (gtv != nullptr && g == 0 && pt.valid) gtv[pt.p] = st_;
    }
  }

  if (PARAMS) {
    double* slab = gslab + (long)blockIdx.x * o.total;
    // wave `wave` owns rows [16 wave, 16 wave + 16) of dVh and dVin
#pragma unroll
    for (int ct = 0; ct < D::MT; ++ct) {
      const int c = 16 * ct + n;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * wave + g + 4 * r;
        if (row < W) {
          if (c < W) slab[o.Vh + row * W + c] = accH[ct][r];
          else if (c == W) slab[o.Vhb + row] = accH[ct][r];
        }
      }
    }
#pragma unroll
    for (int ct = 0; ct < CTG * 4; ++ct) {
      const int c = 16 * ct + n;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * wave + g + 4 * r;
        if (row < W) {
          if (c <= d) slab[o.Vin + row * o.ldin + c] = accIn[ct][r];
          else if (c == d + 1) slab[o.Vinb + row] = accIn[ct][r];
        }
      }
    }
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid <= W) {
      double s = 0.0;
      if (tid < W) {
        const int mt = tid >> 4, gg = tid & 3, r = (tid & 15) >> 2;
        for (int wv = 0; wv < 4; ++wv)
          for (int nn = 0; nn < 16; ++nn) s += sO[(mt * 4 + r) * 256 + wv * 64 + gg * 16 + nn];
        slab[o.Vo + tid] = s;
      } else {
        for (int wv = 0; wv < 4; ++wv)
          for (int nn = 0; nn < 16; ++nn) s += sO[15 * 256 + wv * 64 + nn];
        slab[o.Vob] = s;
      }
    }
  }
}

// the compiled set: width 50, depth 9 (the reference's YAML), [CTG - 1][parameter gradient | input gradient]
typedef void (*BwdKernel)(const double*, const double*, const double*, const double*, const double*, int, int, int, double*,
                          double*, double*);
const BwdKernel bwd_table[2][2] = {{k_disc_bwd<50, 9, 1, true, false>, k_disc_bwd<50, 9, 1, false, true>},
                                   {k_disc_bwd<50, 9, 2, true, false>, k_disc_bwd<50, 9, 2, false, true>}};

// the recomputing kernel of a call: CTG groups of 64 input rows [t; x; 1] (d + 2 <= 128 is the caller's check)
void launch_recompute(bool ingrad, const double* xT, const double* t, const double* tpp, const double* phi, const double* vbar,
                      int N, int L, int d, double* gslab, double* gxv, double* gtv, void* stream) {
  const int ctg = d + 2 <= 64 ? 1 : 2;
  hipLaunchKernelGGL(bwd_table[ctg - 1][ingrad ? 1 : 0], dim3(bwd_blocks((long)N * L)), dim3(256), 0, (hipStream_t)stream, xT, t,
                     tpp, phi, vbar, N, L, d, gslab, gxv, gtv);
}

// the k_disc_rec of a call from the record: NG groups of 48 input rows, TSUM on vertical paths in whole 64-path groups (the input
// layer's gradient once per path group, see k_disc_rec)
struct RecKey {
  int ng;
  bool tsum;
};
RecKey rec_select(int N, int d, bool point_mode, bool tsum_on) {
  return {d + 2 <= 48 ? 1 : d + 2 <= 96 ? 2 : 3, tsum_on && !point_mode && (N % 64) == 0};
}

}  // namespace

extern "C" int xw_disc_bwd_slabs(int N, int L) { return bwd_blocks((long)N * L); }

extern "C" int xw_disc_bwd(const double* xT, const double* t, const double* tpp, const double* phi, const double* vbar,
                           int N, int L, int d, int W, int q, const double* act, double* gslab, void* stream) {
  if (!xT || !phi || !gslab || N <= 0 || L <= 0 || d <= 0) return XW_E_ARG;
  if (!tpp && !t) return XW_E_ARG;
  if (tpp && L != 1) return XW_E_ARG;
  if (!disc_width_ok(W)) return xwg_disc_bwd(xT, t, tpp, phi, vbar, N, L, d, W, q, act, gslab, bwd_blocks((long)N * L), stream);
  // from the record: any depth (the layer loop is rolled -- unrolled for q = 9 it spilled and was 2 % slower); without a
  // record only the recomputing kernel of depth 9 (the reference's YAML) exists
  if (q < 0 || d + 2 > 128 || ((q != 9 || W != 50) && act == nullptr)) return XW_E_DIMS;
  if ((long)N * L * 4 >= (1L << 31)) return XW_E_ARG;
  if (act != nullptr) {
    const RecKey k = rec_select(N, d, tpp != nullptr, xw_switches().disc_rec_tsum != 0);
    return xw_disc_rec_launch(W, k.ng, k.tsum, bwd_blocks((long)N * L), xT, t, tpp, phi, vbar, N, L, d, gslab, act, q, stream);
  }
  launch_recompute(false, xT, t, tpp, phi, vbar, N, L, d, gslab, nullptr, nullptr, stream);
  return xw_launch_status();
}

extern "C" int xw_disc_gradx(const double* xT, const double* t, const double* tpp, const double* phi, const double* vbar,
                             int N, int d, int W, int q, double* gxv, double* gtv, void* stream) {
  if (!xT || !phi || !gxv || N <= 0 || d <= 0) return XW_E_ARG;
  if (!tpp && !t) return XW_E_ARG;
  if (W != 50 || q != 9 || d + 2 > 128) return XW_E_DIMS;
  launch_recompute(true, xT, t, tpp, phi, vbar, N, 1, d, nullptr, gxv, gtv, stream);
  return xw_launch_status();
}
