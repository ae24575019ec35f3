// xw_ode_fwd.h -- the fused stepper's forward pass (xw_ode_core.h has the overview): k_ode_fwd, the narrow-tile forward of the 4x4x4
// form, their table and the width's entry point xw_ode_fwd_multi_w<H>_<K>.  A header, not a source of its own: xw_ode.hip includes it in front of the
// sweeps (xw_ode_<H>_<K>.o), and says why the two are one translation unit.
#pragma once
#ifdef XW_ODE_WIDE16
#include "xw_ode_mfma16.h"
#else
#include "xw_ode_mfma4.h"
#include "xw_ode_n4.h"
#endif

namespace {

// ACT: 0 = no activation store, 1 = the full store, 2 = only what an x-only sweep reads (tanh rows + ReLU mask words)
template <int H, int K, int M, int METHOD, int ACT>
__global__ void __launch_bounds__(64, XW_ODE_FWD_WAVES) k_ode_fwd(const FwdJobs jobs, const double* __restrict__ tf,
                                                const double* __restrict__ th, int L, int d) {
  typedef Dim<H, K> D;
  typedef RK<METHOD> T;
  const int job = find_job(jobs, (int)blockIdx.x);
  const double* __restrict__ xT = jobs.xT[job];
  const double* __restrict__ start = jobs.start[job];
  double* __restrict__ u = jobs.u[job];
  double* __restrict__ Y = jobs.Y[job];
  double* __restrict__ act = jobs.act[job];
  xw_setprio(jobs.prio);
  typedef ActLayout<H, K, M, T::S> AL;
  const int N = jobs.N[job];
  const int lane = xw_lane(), g = lane >> 4, n = lane & 15;
  const int base = ((int)blockIdx.x - jobs.tile0[job]) * 16;
  if (blockIdx.x == 0 && jobs.zero16 != nullptr && lane < 16) jobs.zero16[lane] = 0.0;
  const bool valid = base + n < N;
  const int ncl = valid ? base + n : N - 1;
  const UOff o = u_offsets(d, H, K);
  FieldW<H, K> w;
  load_field<H, K>(th, o, d, w);
  d4 a0[D::HT], a1[D::HT], y[D::HT], flw[D::HT];
  lift<H, K>(th, o, start[ncl], a0, a1, y);
  const d4 xp = project_x<H, K>(th, o, xT, N, d, ncl);
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht) flw[ht] = xw_vecD(th + o.FLw, H, 16 * ht);
  const double flb = th[o.FLb];
  const ActLane aq = act_lane(16, n, true, K);           // every lane of the tile has a slot (padding paths: finite copies)
  const long ntile = (N + 15) >> 4, tile = base >> 4;
  // The checkpoint y_l and u_l leave through buffer descriptors as well (one per time index: rows of [H][N] resp. one row of
  // u): lanes that own nothing -- paths past N in the last tile, rows >= H of the last row tile, the lane groups g > 0 of u --
  // carry an out-of-range offset, so the time loop has no branch but its own (see ActLane.off_part_st).
  const bool big = (long)H * N * 8 >= (1L << 31);         // (a descriptor's 32-bit range: beyond it the plain guarded stores)
  unsigned yoff[4 * D::HT];
#pragma unroll
  for (int ht = 0; ht < D::HT; ++ht)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * ht + g + 4 * r;
      yoff[4 * ht + r] = (valid && row < H) ? 8u * (unsigned)(g * N + base + n) : XW_ACT_OOB;
    }
  const unsigned uoff = (g == 0 && valid) ? 8u * (unsigned)(base + n) : XW_ACT_OOB;
  for (int l = 0; l < L; ++l) {
    double part = 0.0;
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(Y != nullptr && !big ? Y + (long)l * H * N : nullptr, 0,
                                                                         Y != nullptr && !big ? H * N * 8 : 0, 0x00020000);
#pragma unroll
    for (int ht = 0; ht < D::HT; ++ht)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        part += flw[ht][r] * y[ht][r];
        if (16 * ht + 4 * r < H) {                         // (compile time: the register holds live rows)
          const double x = y[ht][r];
          const xw_u2v w2 = {(unsigned)__double2loint(x), (unsigned)__double2hiint(x)};
          __builtin_amdgcn_raw_buffer_store_b64(w2, yrs, (int)yoff[4 * ht + r], (16 * ht + 4 * r) * N * 8, 0);
        }
      }
    if (big && Y != nullptr) {                             // (uniform, never taken below 13 million paths)
#pragma unroll
      for (int ht = 0; ht < D::HT; ++ht)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * ht + g + 4 * r;
          if (valid && row < H) Y[((long)l * H + row) * N + base + n] = y[ht][r];
        }
    }
    const double ul = xw_sum_over_g(part) + flb;           // final_linear, src/model.py:110
    {
      const __amdgpu_buffer_rsrc_t urs = __builtin_amdgcn_make_buffer_rsrc(u + (long)l * N, 0, N * 8, 0x00020000);
      const xw_u2v w2 = {(unsigned)__double2loint(ul), (unsigned)__double2hiint(ul)};
      __builtin_amdgcn_raw_buffer_store_b64(w2, urs, (int)uoff, 0, 0);
    }
    if (l == L - 1) break;
    const double t0 = tf[l], dt = tf[l + 1] - t0;
    d4 k[T::S][D::HT];
#pragma unroll
    for (int i = 0; i < T::S; ++i) {
      d4 yi[D::HT];
#pragma unroll
      for (int ht = 0; ht < D::HT; ++ht) {
        yi[ht] = y[ht];
#pragma unroll
        for (int j = 0; j < i; ++j)
          if (T::a(i, j) != 0.0) yi[ht] += (dt * T::a(i, j)) * k[j][ht];
      }
      if (!ACT) {
        field_fwd<H, K, M, true>(w, t0 + T::c(i) * dt, xp, yi, k[i], SinkNone{});
      } else {
        double* __restrict__ A = act + ((long)l * ntile + tile) * (AL::TOTAL * 16);
        const ActBuf AB = act_buf(A, AL::TOTAL * 16 * 8);
        if (i > 0 && ACT == 1) {
#pragma unroll
          for (int ht = 0; ht < D::HT; ++ht)
            act_store(AB, AL::YI + (i - 1) * H + 16 * ht, H - 16 * ht < 16 ? H - 16 * ht : 16, 16, aq, yi[ht]);
        }
        unsigned bits = 0, bits_hi = 0;
        field_fwd<H, K, M, true>(w, t0 + T::c(i) * dt, xp, yi, k[i], SinkAct<K, M, ACT == 1>{AB, i * AL::STAGE, 16, aq, bits, bits_hi});
        __builtin_amdgcn_raw_buffer_store_b32(bits, AB.rsrc, lane * 4, (AL::MASK + AL::MR * i) * 16 * 8, 0);   // 1 = open (SaveX)
        if (XW_MASK_WORDS(M) == 2) __builtin_amdgcn_raw_buffer_store_b32(bits_hi, AB.rsrc, lane * 4, (AL::MASK + AL::MR * i + 2) * 16 * 8, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < T::S; ++i)
      if (T::b(i) != 0.0)
#pragma unroll
        for (int ht = 0; ht < D::HT; ++ht) y[ht] += (dt * T::b(i)) * k[i][ht];
  }
}

// the compiled set: [depth - 1].k[slot], the slots as choose_fwd counts them (xw_ode_select.h): the narrow tiles first
template <int M, int SLOT> struct FwdAt {
  static constexpr int KIND = SLOT % XW_FWD_KINDS;
  static constexpr OdeKernel<FwdJobs> pick() {
#if XW_ODE_HAS_NARROW
    if constexpr (SLOT < XW_FWD_KINDS) return n4::k_ode_fwd_n4<XW_ODE_H, XW_ODE_K, M, KIND / 3, KIND % 3>;
    else
#endif
      return k_ode_fwd<XW_ODE_H, XW_ODE_K, M, KIND / 3, KIND % 3>;
  }
  static constexpr OdeKernel<FwdJobs> k = pick();
};
const auto fwd_table = kernel_table<FwdAt, FwdJobs, XW_FWD_SLOTS>();

}  // namespace

extern "C" int XW_ODE_FN(xw_ode_fwd_multi_w)(const XwOdeFwdJob* jobs, int njobs, const double* t, const double* theta, int method,
                                             int L, int d, int m, double* zero16, void* stream) {
  if (!jobs || njobs < 1 || njobs > XW_MAXJOBS || !t || !theta || L <= 0 || d <= 0 || m < 1) return XW_E_ARG;
  FwdJobs J;
  J.n = njobs;
  J.zero16 = zero16;
  J.x_only = jobs[0].act_x_only ? 1 : 0;
  J.narrow = jobs[0].narrow ? 1 : 0;
  J.prio = XW_ODE_PRIO - (jobs[0].prio_drop < 0 ? 0 : jobs[0].prio_drop > 3 ? 3 : jobs[0].prio_drop);
  J.tile0[0] = 0;
  for (int i = 0; i < XW_MAXJOBS; ++i) {
    const bool on = i < njobs;
    if (on && (!jobs[i].xT || !jobs[i].start || !jobs[i].u || jobs[i].N <= 0)) return XW_E_ARG;
    if (on && (jobs[i].act_x_only ? 1 : 0) != J.x_only) return XW_E_ARG;         // one store mode per launch
    if (on && (jobs[i].narrow ? 1 : 0) != J.narrow) return XW_E_ARG;              // one layout per launch
    J.xT[i] = on ? jobs[i].xT : nullptr;
    J.start[i] = on ? jobs[i].start : nullptr;
    J.u[i] = on ? jobs[i].u : nullptr;
    J.Y[i] = on ? jobs[i].Y : nullptr;
    J.act[i] = (on && method != 2) ? jobs[i].act : nullptr;     // (rk4 sweeps recompute: nothing to store)
    if (on && (J.act[i] != nullptr) != (J.act[0] != nullptr)) return XW_E_ARG;   // all groups of a launch, or none
    J.N[i] = on ? jobs[i].N : 0;
    J.tile0[i + 1] = J.tile0[i] + (on ? (jobs[i].N + 15) / 16 : 0);
  }
  if (!depth_compiled(m)) return XW_E_DIMS;
  const FwdChoice c = choose_fwd(method, J.act[0] != nullptr, J.x_only != 0, J.narrow != 0);   // (all jobs bring a store, or none: above)
  if (c.rc) return c.rc;
  // (narrow tiles: the same grid of 16-path tiles, four waves of 4 paths each)
  hipLaunchKernelGGL(fwd_table[m - 1].k[c.slot], dim3(J.tile0[J.n]), dim3(c.narrow ? 256 : 64), 0, (hipStream_t)stream, J, t, theta, L, d);
  return xw_launch_status();
}
