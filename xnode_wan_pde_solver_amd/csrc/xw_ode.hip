// xw_ode.hip -- the fused stepper's reverse sweeps (xw_ode_core.h has the overview): sweep_body, k_ode_bwd, k_ode_bwd_duo, the
// narrow-tile sweep of the 4x4x4 form, their table and the width's entry point.  Compiled twice per width (Makefile):
//   xw_ode_<H>_<K>.o          the sweeps from the activation store and xw_ode_bwd_multi_w<H>_<K>, with the forward pass (xw_ode_fwd.h) in
//                             front of them in the SAME translation unit.  The two were meant to be objects of their own; the compiler's
//                             output does not allow it: built without the forward kernels beside them, every sweep kernel here comes out
//                             with another register allocation and schedule (profiles/r24_stepper_by_kernel.md), and the kernels as they
//                             stand are the measured ones.  The forward source first: its kernels stand in front of the sweeps in the
//                             code object (xw_ode_select.h on why the order counts).
//   xw_ode_<H>_<K>_recomp.o   -DXW_ODE_PART_RECOMP: the recomputing sweeps and xw_ode_bwd_recomp_w<H>_<K>, without the forward pass
#ifndef XW_ODE_PART_RECOMP
#include "xw_ode_fwd.h"
#endif
#ifdef XW_ODE_WIDE16
#include "xw_ode_mfma16.h"
#else
#include "xw_ode_mfma4.h"
#include "xw_ode_n4.h"
#endif

// The RECOMPUTING sweeps (no activation store: rk4, adjoint = True, XW_KEEP_ACT=0) are compiled into a second object per width
// (-DXW_ODE_PART_RECOMP): at (32, 12) the largest of them (midpoint / rk4 with weight gradients, the continuous adjoint) crash
// clang 22's 'AMDGPU Rewrite AGPR-Copy-MFMA' pass under -amdgpu-mfma-vgpr-form, which the kernels of the training path want
// (forward, sweeps from the store, narrow tiles: without it the (32, 12) object spilled thousands of registers to scratch).
// jobs: a BwdJobs, by address -- the struct lives in the anonymous namespace (it is part of every sweep kernel's symbol, which must
// not change), so two objects cannot name it in a signature they share.
extern "C" int XW_ODE_FN(xw_ode_bwd_recomp_w)(const void* jobs, const double* t, const double* theta, int method, int L, int d,
                                              int m, int params, int adj, void* stream);

namespace {

// what the reverse of one step l -> l+1 needs from the forward pass: the stage inputs and the stage activations
template <int H, int K, int M, int S> struct Rec {
  d4 yi[S][Dim<H, K>::HT];
  Save<M> sv[S];
};
template <int H, int K>
__device__ __forceinline__ void load_ckpt(const double* __restrict__ Y, int l, int N, int ncl, d4 (&y)[Dim<H, K>::HT]) {
  const int g = xw_lane() >> 4;
#pragma unroll
  for (int ht = 0; ht < Dim<H, K>::HT; ++ht)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * ht + g + 4 * r;
      y[ht][r] = row < H ? Y[((long)l * H + row) * N + ncl] : 0.0;
    }
}
// rebuild the stages of step l -> l+1 from the checkpoint y_l (no dependence on any cotangent)
template <int H, int K, int M, int METHOD>
__device__ __forceinline__ void recompute(const FieldW<H, K>& w, d4 xp, const double* __restrict__ Y,
                                          const double* __restrict__ tf, int l, int N, int ncl,
                                          Rec<H, K, M, RK<METHOD>::S>& R) {
  typedef Dim<H, K> D;
  typedef RK<METHOD> T;
  const double t0 = tf[l], dt = tf[l + 1] - t0;
  d4 k[T::S][D::HT];
  load_ckpt<H, K>(Y, l, N, ncl, R.yi[0]);
#pragma unroll
  for (int i = 0; i < T::S; ++i) {
    if (i > 0) {
#pragma unroll
      for (int ht = 0; ht < D::HT; ++ht) {
        R.yi[i][ht] = R.yi[0][ht];
#pragma unroll
        for (int j = 0; j < i; ++j)
          if (T::a(i, j) != 0.0) t_axpy(R.yi[i][ht], dt * T::a(i, j), k[j][ht], D::HR(ht));
      }
    }
    if (i < T::S - 1)
      field_fwd<H, K, M, true>(w, t0 + T::c(i) * dt, xp, R.yi[i], k[i], SinkSave<M>{R.sv[i]});
    else
      field_fwd<H, K, M, false>(w, t0 + T::c(i) * dt, xp, R.yi[i], k[i], SinkSave<M>{R.sv[i]});   // last stage: activations only
  }
}

// one stage of that record read back from the forward pass's activation store (k_ode_fwd<ACT>): loads only.
// Stage granularity: while one stage is reversed the loads of the next one are in flight -- a whole step ahead would
// keep twice as many registers occupied.
template <int H, int K, int M, class SV = Save<M>> struct StageRec {
  d4 yi[Dim<H, K>::HT];        // (not loaded for SaveX: a sweep without weight gradients never reads the stage input)
  SV sv;
};
template <int H, int K, int M, int METHOD, class SV>
__device__ __forceinline__ void load_stage(const double* __restrict__ Y, const double* __restrict__ act, int l, int i,
                                           int N, int ncl, StageRec<H, K, M, SV>& R) {
  typedef Dim<H, K> D;
  typedef ActLayout<H, K, M, RK<METHOD>::S> AL;
  const long ntile = (N + 15) >> 4, tile = __builtin_amdgcn_readfirstlane(ncl >> 4);   // (clamped lanes stay in the tile)
  const double* __restrict__ A = act + ((long)l * ntile + tile) * (AL::TOTAL * 16);
  const ActLane q = act_lane(16, xw_lane() & 15, true, K);
  if constexpr (std::is_same<SV, SaveX<M>>::value) {
    R.sv.bits = reinterpret_cast<const unsigned*>(A + (AL::MASK + AL::MR * i) * 16)[xw_lane()];
    R.sv.bits_hi = XW_MASK_WORDS(M) == 2 ? reinterpret_cast<const unsigned*>(A + (AL::MASK + AL::MR * i + 2) * 16)[xw_lane()] : 0u;
    R.sv.a = act_load(A, i * AL::STAGE + (M - 1) * K, K, 16, q);
    return;
  }
  if (i == 0) {
    load_ckpt<H, K>(Y, l, N, ncl, R.yi);
  } else {
#pragma unroll
    for (int ht = 0; ht < D::HT; ++ht)
      R.yi[ht] = act_load(A, AL::YI + (i - 1) * H + 16 * ht, H - 16 * ht < 16 ? H - 16 * ht : 16, 16, q);
  }
  if constexpr (std::is_same<SV, Save<M>>::value) {
#pragma unroll
    for (int j = 0; j < M - 1; ++j) R.sv.z[j] = act_load(A, i * AL::STAGE + j * K, K, 16, q);
    R.sv.a = act_load(A, i * AL::STAGE + (M - 1) * K, K, 16, q);
  }
}

// SAVED: the stage activations come from the forward pass's store (euler, midpoint); otherwise they are recomputed
// ADJ: the reference's adjoint=True (src/model.py:103: torchdiffeq.odeint_adjoint) -- not the reverse of the steps that
//   were taken but the continuous adjoint, integrated with the same fixed-grid method.  torchdiffeq 0.1.1 (absent here,
//   restated from its published OdeintAdjointMethod.backward): for i = L-1 .. 1 the augmented state (y, a, theta-bar) starts
//   from the FORWARD solution y(t_i) and takes ONE step of `method` from t_i to t_{i-1} (h < 0) under
//       d/dt (y, a, theta-bar) = ( f(t, y), -a^T df/dy, -a^T df/dtheta ),
//   then a += the cotangent of y(t_{i-1}).  Its parameter set is the field module's parameters; the sample point x is a
//   plain attribute of that module, so no gradient reaches x through the field (only through the start value).
// DUO (with PARAMS and SAVED): the "duo" sweep.  This wave runs the adjoint chain exactly like the sweep without weight
//   gradients (ReLU mask words + tanh rows from the store) and posts the cotangent tiles of every field evaluation into
//   one of two alternating LDS buffers (qbuf); a second wave of the block (duo_outer) contracts them with the layer
//   inputs, which it loads from the activation store directly in operand layout -- one workgroup barrier per field
//   evaluation.  One wave per 16 paths left three quarters of the SIMDs idle at N = 4096 and bound the sweep by the
//   latency of ONE instruction stream (chain, LDS round trips, loads); the split doubles the waves and halves the stream.
template <int H, int K, int M, int METHOD, bool PARAMS, bool SAVED, bool ADJ, bool DUO>
__device__ __forceinline__ void sweep_body(const BwdJobs& jobs, const double* __restrict__ tf, const double* __restrict__ th,
                                           int L, int d, double* lds, double* qbuf, int vb) {
  static_assert(!SAVED || RK<METHOD>::S <= 2, "the activation store is used by euler and midpoint");
  static_assert(!(SAVED && ADJ), "the continuous adjoint evaluates the field at its own stage points");
  static_assert(!DUO || (PARAMS && SAVED), "the duo sweep is the sweep with weight gradients from the activation store");
  typedef Dim<H, K> D;
  typedef RK<METHOD> T;
  constexpr int OUTER = DUO ? 2 : (PARAMS ? 1 : 0);
  xw_setprio(jobs.prio);
  int qflip = 0;                                 // DUO: which of the two Q buffers the next field evaluation posts into
  if (PARAMS && !DUO) {
    if (xw_lane() < 16) lds[2 * XW_TTILE + K * XW_TSTRIDE + xw_lane()] = 1.0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  const int job = find_job(jobs, vb);
  const double* __restrict__ xT = jobs.xT[job];
  const double* __restrict__ start = jobs.start[job];
  const double* __restrict__ Y = jobs.Y[job];
  const double* __restrict__ act = jobs.act[job];
  const double* __restrict__ ubar = jobs.ubar[job];
  double* __restrict__ gx = jobs.gx[job];
  double* __restrict__ gs = jobs.gs[job];
  double* __restrict__ gslab = jobs.gslab[job];
  const int N = jobs.N[job];
  const int tile = vb - jobs.tile0[job];
  const int lane = xw_lane(), g = lane >> 4, n = lane & 15;
  const int base = tile * 16;
  const bool valid = base + n < N;
  const int ncl = valid ? base + n : N - 1;
  const UOff o = u_offsets(d, H, K);
  FieldW<H, K> w;                               // (only the recomputing paths load it)
  FieldWT<H, K> wT;
  load_field_T<H, K>(th, o, d, wT);
  d4 flw[D::HT];
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) flw[ht] = xw_vecD(th + o.FLw, H, 16 * ht);

  FieldG<H, K> G;
  G.Wh = xw_zero4();
#pragma unroll
  for (int ct = 0; ct < (H + 1 + 15) / 16; ++ct) G.Wy[ct] = xw_zero4();
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) G.Wo[ht] = xw_zero4();
  d4 accFL[D::HT];
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) accFL[ht] = xw_zero4();
  double accFLb = 0.0;
  d4 lam[D::HT];
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) lam[ht] = xw_zero4();
  d4 xpb = xw_zero4();
  double ub0 = 0.0;            // cotangent of u at the first time index (the last one visited)

  // read-out u_l = FL y_l + b at time index l: cotangent into lam, gradients of the read-out layer
  // cotangent of u at time index l.  Loaded at the START of the step that ends with its read-out: behind the fences of
  // the outer products the load could not be hoisted and its HBM latency sat on the chain once per step.
  auto load_ub = [&](int l) -> double {
    return valid ? cot_u(jobs, job, ubar, l, N, base + n, L) : 0.0;
  };
  auto readout = [&](int l, const d4 (&yl)[D::HT], double ub) {
    ub0 = ub;
#pragma unroll
    for (int ht = 0; ht < D::HT; ++ht) {
      t_axpy(lam[ht], ub, flw[ht], D::HR(ht));
      if (PARAMS) t_axpy(accFL[ht], ub, yl[ht], D::HR(ht));
    }
    if (PARAMS) accFLb += ub;
  };
  // reverse of ONE stage i of the step l -> l+1: kb[i] is the cotangent of the stage derivative k_i
  d4 kb[T::S][D::HT], psum[D::HT];
  auto begin_step = [&](int l) {
    const double dt = tf[l + 1] - tf[l];
#pragma unroll
    for (int i = 0; i < T::S; ++i)
#pragma unroll
      for (int ht = 0; ht < D::HT; ++ht) {
        t_scale(kb[i][ht], dt * T::b(i), lam[ht], D::HR(ht));
        if (i == 0) psum[ht] = xw_zero4();
      }
  };
  auto reverse_stage = [&](int l, int i, const d4 (&yin)[D::HT], const auto& sv) {
    const double t0 = tf[l], dt = tf[l + 1] - t0;
    d4 psi[D::HT];
    field_vjp<H, K, M, OUTER>(w, wT, t0 + T::c(i) * dt, sv, yin, kb[i], psi, xpb, G,
                              DUO ? qbuf + qflip * DuoPlan<H, K, M>::BUF : lds);
    if (DUO) {      // the tiles of this evaluation are complete: hand them over (the partner is one evaluation behind)
      // (LDS only: a workgroup-scope release fence would also drain vmcnt, i.e. wait for the next stage's prefetch loads)
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      qflip ^= 1;
    }
#pragma unroll
    for (int ht = 0; ht < D::HT; ++ht) {
      t_add(psum[ht], psi[ht], D::HR(ht));
#pragma unroll
      for (int j = 0; j < T::S; ++j)
        if (j < i && T::a(i, j) != 0.0) t_axpy(kb[j][ht], dt * T::a(i, j), psi[ht], D::HR(ht));
    }
  };
  auto end_step = [&](int l, const d4 (&y_l)[D::HT], double ub) {
#pragma unroll
    for (int ht = 0; ht < D::HT; ++ht) t_add(lam[ht], psum[ht], D::HR(ht));
    readout(l, y_l, ub);
  };

  if constexpr (ADJ) {
    load_field<H, K>(th, o, d, w);
    const d4 xp = project_x<H, K>(th, o, xT, N, d, ncl);
    {
      d4 yl[D::HT];
      load_ckpt<H, K>(Y, L - 1, N, ncl, yl);
      readout(L - 1, yl, load_ub(L - 1));
    }
    for (int l = L - 2; l >= 0; --l) {
      const double ub = load_ub(l);
      const double t1 = tf[l + 1], dt = t1 - tf[l];             // the step goes from t1 back to t1 - dt
      d4 y1[D::HT];
      load_ckpt<H, K>(Y, l + 1, N, ncl, y1);
      d4 ky[T::S][D::HT], ps[T::S][D::HT], asum[D::HT];          // stage derivatives of y; a_s^T df/dy; update of the adjoint
#pragma unroll
      for (int ht = 0; ht < D::HT; ++ht) asum[ht] = xw_zero4();
#pragma unroll
      for (int i = 0; i < T::S; ++i) {
        d4 ys[D::HT], as[D::HT];
#pragma unroll
        for (int ht = 0; ht < D::HT; ++ht) {
          ys[ht] = y1[ht];
          as[ht] = lam[ht];
#pragma unroll
          for (int j = 0; j < i; ++j)
            if (T::a(i, j) != 0.0) {
              ys[ht] -= (dt * T::a(i, j)) * ky[j][ht];           // h = -dt;  dy/dt = f
              as[ht] += (dt * T::a(i, j)) * ps[j][ht];           //           da/dt = -a^T df/dy
            }
        }
        const double ti = t1 - T::c(i) * dt;
        Save<M> sv;
        field_fwd<H, K, M, true>(w, ti, xp, ys, ky[i], SinkSave<M>{sv});
        if (T::b(i) != 0.0) {
          // this stage enters the update: the vector-Jacobian product is taken of (dt b_i) a_s, so that the weight-gradient
          // outer products inside it accumulate  -h b_i a_s^T df/dtheta  directly
          d4 cot[D::HT], psi[D::HT];
#pragma unroll
          for (int ht = 0; ht < D::HT; ++ht) cot[ht] = (dt * T::b(i)) * as[ht];
          field_vjp<H, K, M, PARAMS ? 1 : 0>(w, wT, ti, sv, ys, cot, psi, xpb, G, lds);
#pragma unroll
          for (int ht = 0; ht < D::HT; ++ht) {
            asum[ht] += psi[ht];
            ps[i][ht] = (1.0 / (dt * T::b(i))) * psi[ht];
          }
        } else {
          d4 xdummy = xw_zero4();
          FieldG<H, K> Gd;                                       // (untouched: no parameter products in this call)
          field_vjp<H, K, M, 0>(w, wT, ti, sv, ys, as, ps[i], xdummy, Gd, lds);
        }
      }
#pragma unroll
      for (int ht = 0; ht < D::HT; ++ht) lam[ht] += asum[ht];
      d4 yl[D::HT];
      load_ckpt<H, K>(Y, l, N, ncl, yl);
      readout(l, yl, ub);
    }
  } else if constexpr (SAVED) {
    // (without weight gradients the sweep only needs tanh(z_{m-1}) and the ReLU masks of a stage)
    // (the duo sweep's chain wave neither: its partner reads the layer inputs)
    typedef typename std::conditional<PARAMS && !DUO, Save<M>, SaveX<M>>::type SV;
    // y_l for the read-out layer's weight gradient: the stage-0 record carries it, except in the duo sweep
    auto y_of = [&](int l, const d4 (&rec)[D::HT], d4 (&yl)[D::HT]) {
      if (DUO) load_ckpt<H, K>(Y, l, N, ncl, yl);
      else {
#pragma unroll
        for (int ht = 0; ht < D::HT; ++ht) yl[ht] = rec[ht];
      }
    };
    // The cotangent of u is requested ONE STEP AHEAD by straight-line code (Cot4 above), in front of the stage record's
    // requests: cot_u's branches wait for their loads where they stand (vmcnt(0)), which drained the record prefetched for the
    // next stage -- one exposed memory latency per step in every sweep whose cotangent is formed from a residual (the
    // boundary sweep, sweep B).
    const Cot4 cot = make_cot(jobs, job, N, ncl, valid, Y);
    auto run = [&](auto weak_tag) {
      constexpr bool WEAK = decltype(weak_tag)::value;
      StageRec<H, K, M, SV> sa, sb;
      const CotRaw raw_last = cot_issue<WEAK>(cot, L - 1);
      CotRaw raw = cot_issue<WEAK>(cot, L > 1 ? L - 2 : 0);
      if constexpr (T::S == 2) {
        // stage 1 always lives in sa, stage 0 in sb: each is loaded while the other one is reversed
        if (L > 1) load_stage<H, K, M, METHOD>(Y, act, L - 2, 1, N, ncl, sa);
      } else {
        if (L > 1) load_stage<H, K, M, METHOD>(Y, act, L - 2, 0, N, ncl, sa);
      }
      {
        d4 yl[D::HT];
        load_ckpt<H, K>(Y, L - 1, N, ncl, yl);
        readout(L - 1, yl, cot_value<WEAK>(cot, raw_last, L - 1, L));
      }
      if constexpr (T::S == 2) {
        for (int l = L - 2; l >= 0; --l) {
          const double ub = cot_value<WEAK>(cot, raw, l, L);       // (requested a step ago)
          d4 yl[D::HT];
          load_stage<H, K, M, METHOD>(Y, act, l, 0, N, ncl, sb);
          raw = cot_issue<WEAK>(cot, l > 0 ? l - 1 : 0);
          y_of(l, sb.yi, yl);
          begin_step(l);
          reverse_stage(l, 1, sa.yi, sa.sv);
          load_stage<H, K, M, METHOD>(Y, act, l > 0 ? l - 1 : 0, 1, N, ncl, sa);
          reverse_stage(l, 0, sb.yi, sb.sv);
          end_step(l, yl, ub);                              // stage 0's input is y_l itself
        }
      } else {
        for (int l = L - 2; l >= 0; --l) {
          const double ub = cot_value<WEAK>(cot, raw, l, L);
          d4 yl[D::HT];
          sb = sa;
          raw = cot_issue<WEAK>(cot, l > 0 ? l - 1 : 0);
          load_stage<H, K, M, METHOD>(Y, act, l > 0 ? l - 1 : 0, 0, N, ncl, sa);
          y_of(l, sb.yi, yl);
          begin_step(l); reverse_stage(l, 0, sb.yi, sb.sv); end_step(l, yl, ub);
        }
      }
    };
    if (cot.weak) run(std::true_type{});
    else run(std::false_type{});
  } else if constexpr (T::S <= 2) {
    load_field<H, K>(th, o, d, w);
    const d4 xp = project_x<H, K>(th, o, xT, N, d, ncl);
    Rec<H, K, M, T::S> cur;
    {
      d4 yl[D::HT];
      load_ckpt<H, K>(Y, L - 1, N, ncl, yl);
      readout(L - 1, yl, load_ub(L - 1));
    }
    for (int l = L - 2; l >= 0; --l) {
      const double ub = load_ub(l);
      recompute<H, K, M, METHOD>(w, xp, Y, tf, l, N, ncl, cur);
      begin_step(l);
#pragma unroll
      for (int i = T::S - 1; i >= 0; --i) reverse_stage(l, i, cur.yi[i], cur.sv[i]);
      end_step(l, cur.yi[0], ub);
    }
  } else {
    load_field<H, K>(th, o, d, w);
    const d4 xp = project_x<H, K>(th, o, xT, N, d, ncl);
    for (int l = L - 1; l >= 0; --l) {
      d4 y[D::HT];
  #pragma unroll
      for (int ht = 0; ht < D::HT; ++ht)
  #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * ht + g + 4 * r;
          y[ht][r] = row < H ? Y[((long)l * H + row) * N + ncl] : 0.0;
        }
      if (l < L - 1) {
        // reverse of the step l -> l+1 : lam currently holds the total cotangent of y_{l+1}
        const double t0 = tf[l], dt = tf[l + 1] - t0;
        d4 k[T::S][D::HT], kb[T::S][D::HT], psum[D::HT];
        Save<M> sv;
  #pragma unroll
        for (int i = 0; i < T::S - 1; ++i) {      // stage derivatives needed to rebuild the later stage inputs
          d4 yi[D::HT];
  #pragma unroll
          for (int ht = 0; ht < D::HT; ++ht) {
            yi[ht] = y[ht];
  #pragma unroll
            for (int j = 0; j < i; ++j)
              if (T::a(i, j) != 0.0) yi[ht] += (dt * T::a(i, j)) * k[j][ht];
          }
          field_fwd<H, K, M, true>(w, t0 + T::c(i) * dt, xp, yi, k[i], SinkNone{});
        }
  #pragma unroll
        for (int i = 0; i < T::S; ++i)
  #pragma unroll
          for (int ht = 0; ht < D::HT; ++ht) {
            kb[i][ht] = (dt * T::b(i)) * lam[ht];
            if (i == 0) psum[ht] = xw_zero4();
          }
  #pragma unroll
        for (int i = T::S - 1; i >= 0; --i) {
          d4 yi[D::HT], ko[D::HT], psi[D::HT];
  #pragma unroll
          for (int ht = 0; ht < D::HT; ++ht) {
            yi[ht] = y[ht];
  #pragma unroll
            for (int j = 0; j < i; ++j)
              if (T::a(i, j) != 0.0) yi[ht] += (dt * T::a(i, j)) * k[j][ht];
          }
          const double ti = t0 + T::c(i) * dt;
          field_fwd<H, K, M, true>(w, ti, xp, yi, ko, SinkSave<M>{sv});
          field_vjp<H, K, M, PARAMS ? 1 : 0>(w, wT, ti, sv, yi, kb[i], psi, xpb, G, lds);
  #pragma unroll
          for (int ht = 0; ht < D::HT; ++ht) {
            psum[ht] += psi[ht];
  #pragma unroll
            for (int j = 0; j < i; ++j)
              if (T::a(i, j) != 0.0) kb[j][ht] += (dt * T::a(i, j)) * psi[ht];
          }
        }
  #pragma unroll
        for (int ht = 0; ht < D::HT; ++ht) lam[ht] += psum[ht];
      }
      // read-out u_l = FL y_l + b
      const double ub = valid ? cot_u(jobs, job, ubar, l, N, base + n, L) : 0.0;
      ub0 = ub;
  #pragma unroll
      for (int ht = 0; ht < D::HT; ++ht) {
        lam[ht] += flw[ht] * ub;
        if (PARAMS) accFL[ht] += y[ht] * ub;
      }
      if (PARAMS) accFLb += ub;
    }
  }

  // (duo sweep: the three transpose tiles of the epilogue live in the Q buffer that is NOT in flight -- the partners are
  //  reading the one the last evaluation was posted into; they finished with the other one before the last barrier)
  if (DUO) lds = qbuf + qflip * DuoPlan<H, K, M>::BUF;
  double* slab = PARAMS ? gslab + (long)tile * o.total : nullptr;
  sweep_tail<H, K, PARAMS, ADJ>(th, o, d, N, base, valid, ncl, xT, start[ncl], jobs.x_ones != 0, lam, xpb, ub0, accFL, accFLb, flw,
                                gx, gs, slab, lds, [&]() {
                                  if (PARAMS && !DUO) store_field_grads<H, K>(slab, o, d, G);   // (duo sweep: the partner wave stores them)
                                });
}

template <int H, int K, int M, int METHOD, bool PARAMS, bool SAVED, bool ADJ = false>
__global__ void __launch_bounds__(64) k_ode_bwd(const BwdJobs jobs, const double* __restrict__ tf,
                                                const double* __restrict__ th, int L, int d) {
  __shared__ double lds[XW_SWEEP_TILES * XW_TTILE];   // (plan: XW_SWEEP_TILES)
  sweep_body<H, K, M, METHOD, PARAMS, SAVED, ADJ, false>(jobs, tf, th, L, d, lds, nullptr, (int)blockIdx.x);
}
// the duo sweep: wave 0 = adjoint chain, wave 1 = weight gradients of the field (see sweep_body / duo_outer).
// Placement (tools/probe_place.hip, profiles/r02_probe_place.txt): the dispatcher puts a block's waves on consecutive
// SIMDs and starts the next block of the same CU ONE SIMD further, so two of these blocks on a CU land on SIMDs (0,1),
// (1,2).  Both remedies were built and measured at 1 / 2 / 3 concurrent jobs of 4096 paths (this form: 105 / 147 / 170 us):
// a spacer wave that ends at once (blocks on (0,2), (1,3); but a block then needs three waves' registers to start, two
// blocks per CU instead of four): 105 / 142 / 181 us, generator sub-step 0.572 ms against 0.518; two tiles per four-wave
// block (every SIMD of the CU, tiles coupled through the block barrier, a job on half the CUs): 118 / 126 / 216 us,
// generator sub-step 0.533 ms.  Two tiles on one CU slow each other by a quarter wherever their waves sit.
#define XW_DUO_THREADS 128
template <int H, int K, int M, int METHOD>
__global__ void __launch_bounds__(XW_DUO_THREADS) k_ode_bwd_duo(const BwdJobs jobs, const double* __restrict__ tf,
                                                                const double* __restrict__ th, int L, int d) {
  __shared__ double lds[2 * DuoPlan<H, K, M>::BUF];
  // jobs.spread (= the chip's CU count, 0: off): every second ROUND of blocks is a spacer that ends at once.  The dispatcher deals
  // blocks round-robin over the CUs and starts a CU's next block one SIMD further than the last (profiles/r02_probe_place.txt):
  // two of these two-wave blocks on a CU sit on SIMDs (0, 1) and (1, 2) -- one SIMD hosts a chain wave AND a partner wave, one
  // stands idle, and a launch of 512 tiles takes 142 us where 256 take 92.  With a spacer round in between the second block
  // starts on SIMD 2: (0, 1), (2, 3).
  int vb = (int)blockIdx.x;
  if (jobs.spread > 0) {
    const int round = vb / jobs.spread;
    if (round & 1) return;
    vb -= (round >> 1) * jobs.spread;
    if (vb >= jobs.tile0[jobs.n]) return;
  }
  if (threadIdx.x < 64) sweep_body<H, K, M, METHOD, true, true, false, true>(jobs, tf, th, L, d, nullptr, lds, vb);
  else duo_outer<H, K, M, METHOD>(jobs, tf, th, L, d, lds, vb);
}

// the compiled sets: [depth - 1].k[slot], the slots as choose_sweep / recomp_slot count them (xw_ode_select.h)
#ifndef XW_ODE_PART_RECOMP
template <int M, int SLOT> struct SweepAt {
  static constexpr int S16 = SLOT - XW_SWEEP_FIRST16;      // among the 16-path kernels: duo, x-only, duo, x-only
  static constexpr OdeKernel<BwdJobs> pick() {
#if XW_ODE_HAS_NARROW
    if constexpr (S16 < 0 || S16 >= 4) return n4::k_ode_bwd_n4<XW_ODE_H, XW_ODE_K, M, SLOT % 2, S16 < 0>;
    else
#endif
    if constexpr (S16 % 2 == 0) return k_ode_bwd_duo<XW_ODE_H, XW_ODE_K, M, S16 / 2>;
    else return k_ode_bwd<XW_ODE_H, XW_ODE_K, M, S16 / 2, false, true>;
  }
  static constexpr OdeKernel<BwdJobs> k = pick();
};
const auto sweep_table = kernel_table<SweepAt, BwdJobs, XW_SWEEP_SLOTS>();
#ifndef XW_ODE_WIDE16     // (the wide container's duo sweep: one block per tile, no spacer round, spread = 0)
// the chip's CU count for the duo sweep's placement: read at the first duo launch of this object, then frozen for the process (the
// switch of the spacer round, duo_spread of xnwan_switches.h, is read at every duo launch)
int duo_placement() {
  static const int ncu = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0;
    return n;
  }();
  return ncu;
}
#endif
#else
template <int M, int SLOT> struct RecompAt {
  static constexpr OdeKernel<BwdJobs> k = k_ode_bwd<XW_ODE_H, XW_ODE_K, M, SLOT / 4, (SLOT / 2) % 2 != 0, false, SLOT % 2 != 0>;
};
const auto recomp_table = kernel_table<RecompAt, BwdJobs, XW_RECOMP_SLOTS>();
#endif

#include "xw_generic_cot.h"  // (the host's check of a sweep job, sweep_job_ok; the cotangent's device text there is not used here)
}  // namespace

#ifndef XW_ODE_PART_RECOMP
extern "C" int XW_ODE_FN(xw_ode_bwd_multi_w)(const XwOdeBwdJob* jobs, int njobs, const double* t, const double* theta, int method,
                                             int L, int d, int m, int mode, void* stream) {
  if (!jobs || njobs < 1 || njobs > XW_MAXJOBS || !t || !theta || L <= 0 || d <= 0 || m < 1 || (mode & 3) == 0 || ((mode & 4) && (mode & 3) != 3) || ((mode & 8) && (mode & 4)) || ((mode & 16) && (mode & 8)) || (mode & ~127)) return XW_E_ARG;
  BwdJobs J;
  J.n = njobs;
  J.x_ones = (mode & 4) ? 1 : 0;
  J.spread = 0;
  J.prio = XW_ODE_PRIO - ((mode >> 5) & 3);
  J.tile0[0] = 0;
  for (int i = 0; i < XW_MAXJOBS; ++i) {
    const bool on = i < njobs;
    if (on && (!jobs[i].Y || !sweep_job_ok(jobs[i], mode))) return XW_E_ARG;      // (xw_generic_cot.h: as every family's entry point)
    if (on && (mode & 1) && (!jobs[i].gx != !jobs[i].gs)) return XW_E_ARG;
    J.xT[i] = on ? jobs[i].xT : nullptr;
    J.start[i] = on ? jobs[i].start : nullptr;
    J.Y[i] = on ? jobs[i].Y : nullptr;
    J.act[i] = (on && method != 2 && !(mode & 8)) ? jobs[i].act : nullptr;   // (rk4 and the continuous adjoint recompute)
    if (on && (J.act[i] != nullptr) != (J.act[0] != nullptr)) return XW_E_ARG;   // all groups of a launch, or none
    J.ubar[i] = on ? jobs[i].ubar : nullptr;
    J.res_u[i] = on ? jobs[i].res_u : nullptr;
    J.res_ref[i] = on ? jobs[i].res_ref : nullptr;
    J.res_coef[i] = on ? jobs[i].res_coef : 0.0;
    J.res_base[i] = on ? jobs[i].res_base : 0.0;
    J.res_first[i] = on ? jobs[i].res_first_only : 0;
    J.res_w[i] = on ? jobs[i].res_w : nullptr;
    J.res_c[i] = on ? jobs[i].res_c : nullptr;
    J.res_cp[i] = on ? jobs[i].res_cp : nullptr;
    J.res_kappa2[i] = on ? jobs[i].res_kappa2 : 0.0;
    J.res_wpp[i] = on ? jobs[i].res_w_per_point : 0;
    J.res_scal[i] = on ? jobs[i].res_scal : nullptr;
    J.res_refA[i] = on ? jobs[i].res_refA : nullptr;
    J.res_coefA[i] = on ? jobs[i].res_coefA : 0.0;
    J.res_baseA[i] = on ? jobs[i].res_baseA : 0.0;
    J.gx[i] = (on && (mode & 1)) ? jobs[i].gx : nullptr;
    J.gs[i] = (on && (mode & 1)) ? jobs[i].gs : nullptr;
    J.gslab[i] = (on && (mode & 2)) ? jobs[i].gslab : nullptr;
    J.N[i] = on ? jobs[i].N : 0;
    J.tile0[i + 1] = J.tile0[i] + (on ? (jobs[i].N + 15) / 16 : 0);
  }
  if (!depth_compiled(m)) return XW_E_DIMS;
  const SweepChoice c = choose_sweep(method, mode, J.act[0] != nullptr);   // (all jobs bring a store, or none: above)
  if (c.rc) return c.rc;
  if (c.kind == SWEEP_RECOMP)
    return XW_ODE_FN(xw_ode_bwd_recomp_w)(&J, t, theta, method, L, d, m, (mode & 2) ? 1 : 0, (mode & 8) ? 1 : 0, stream);
  // one wave per 16-path tile; the duo sweep: chain wave + partner wave; narrow tiles: four waves of 4 paths each
  const int tiles = J.tile0[J.n];
  dim3 grid(tiles);
  const dim3 block(c.kind == SWEEP_DUO ? XW_DUO_THREADS : c.kind == SWEEP_N4 ? 256 : 64);
#ifndef XW_ODE_WIDE16
  if (c.kind == SWEEP_DUO) {
    const DuoGrid g = duo_grid(tiles, duo_placement(), xw_switches().duo_spread != 0);
    J.spread = g.spread;
    grid = dim3(g.blocks);
  }
#endif
  hipLaunchKernelGGL(sweep_table[m - 1].k[c.slot], grid, block, 0, (hipStream_t)stream, J, t, theta, L, d);
  return xw_launch_status();
}
#else   // XW_ODE_PART_RECOMP: only the sweeps that re-evaluate the field (no activation store) and the continuous adjoint
extern "C" int XW_ODE_FN(xw_ode_bwd_recomp_w)(const void* jobs_, const double* t, const double* theta, int method, int L, int d,
                                              int m, int params, int adj, void* stream) {
  const BwdJobs& jobs = *static_cast<const BwdJobs*>(jobs_);
  if (!depth_compiled(m)) return XW_E_DIMS;
  const int slot = recomp_slot(method, params != 0, adj != 0);
  if (slot < 0) return XW_E_ARG;
  hipLaunchKernelGGL(recomp_table[m - 1].k[slot], dim3(jobs.tile0[jobs.n]), dim3(64), 0, (hipStream_t)stream, jobs, t, theta, L, d);
  return xw_launch_status();
}
#endif
