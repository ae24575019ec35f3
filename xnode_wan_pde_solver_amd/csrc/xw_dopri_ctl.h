// xw_dopri_ctl.h -- what the two implementations of solver 'dopri5' share (xw_dopri.hip: the field per path on the vector ALU;
// xw_tdopri.hip: the field per 16-path tile on the matrix pipe): the controller slots, the Dormand-Prince tableau, the dense
// output, the job pack of a launch, the per-job ticket reduction, the step controller (ctl_init1 / ctl_init2 / ctl_attempt: what the
// lane that job_sum returns true on does with the totals) and the host side's job checks.  xw_tdopri_paths.hip, a controller per
// PATH, takes the tableau, the dense output and the controller's formulas by value (ctl_h0 / ctl_first_dt / ctl_next_dt).  What stays with each implementation is
// how a block or a tile forms its partial sums and where its vectors live.  Library-internal; included INSIDE an anonymous
// namespace, after xw_generic_cot.h and after a gsum64(double) (the sum over the wave) has been declared.
#pragma once

// controller slots (include/xnwan.h)
enum { C_T0 = 0, C_DT = 1, C_NACC = 2, C_NATT = 3, C_DONE = 4, C_STATUS = 5, C_H0 = 6, C_D1 = 7, C_RATIO = 8, C_GAP = 9, C_TICKET = 15 };

// Dormand-Prince 5(4) (torchdiffeq _DORMAND_PRINCE_SHAMPINE_TABLEAU, DPS_C_MID): nodes, stage rows (row s feeds stage s from
// k_0 .. k_{s-1}; row 6 is the 5th-order solution, FSAL), error weights b - b^, and the weights of the midpoint of the dense output
__constant__ double DP_C[7] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
__constant__ double DP_A[7][6] = {
    {0, 0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0},
    {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}};
__constant__ double DP_B[7] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84, 0};
__constant__ double DP_E[7] = {35.0 / 384 - 1951.0 / 21600, 0, 500.0 / 1113 - 22642.0 / 50085, 125.0 / 192 - 451.0 / 720,
                               -2187.0 / 6784 + 12231.0 / 42400, 11.0 / 84 - 649.0 / 6300, -1.0 / 60};
__constant__ double DP_MID[7] = {6025192743.0 / 30085553152 / 2, 0, 51252292925.0 / 65400821598 / 2,
                                 -2691868925.0 / 45128329728 / 2, 187940372067.0 / 1594534317056 / 2,
                                 -1776094331.0 / 19743644256 / 2, 11237099.0 / 235043384 / 2};
constexpr double DP_SAFETY = 0.9, DP_IFACTOR = 10.0, DP_DFACTOR = 0.2;

// The dense output is the quartic through y0, y1 (x = 1), y_mid (x = 1/2) with slopes dt f0, dt f1 (torchdiffeq _interp_fit):
// with y1 and y_mid linear in the stages it is p(x) = y0 + dt sum_j w_j(x) k_j, w_j(x) below (w_j(1) = b_j)
__device__ __forceinline__ void dense_weights(double x, double (&w)[7]) {
  const double x2 = x * x, x3 = x2 * x, x4 = x3 * x;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const double b = DP_B[j], cm = DP_MID[j];
    const double d0 = j == 0 ? 1.0 : 0.0, d6 = j == 6 ? 1.0 : 0.0;
    w[j] = x * d0 + x2 * (d6 - 4 * d0 - 5 * b + 16 * cm) + x3 * (5 * d0 - 3 * d6 + 14 * b - 32 * cm) +
           x4 * (2 * d6 - 2 * d0 - 8 * b + 16 * cm);
  }
}

#define XW_DOPRI_MAXJOBS 8
template <class J> struct Jobs {
  J j[XW_DOPRI_MAXJOBS];
  int blk0[XW_DOPRI_MAXJOBS + 1];    // first block of every job: prefix sums of the jobs' block counts (fwd_jobs / sweep_jobs;
                                     // a block is 64 paths in xw_dopri.hip, one 16-path tile in xw_tdopri.hip)
  int njobs;
};
template <class J> __device__ __forceinline__ int job_of(const Jobs<J>& J_, int& lb) {
  int jb = 0;
  while (jb + 1 < J_.njobs && (int)blockIdx.x >= J_.blk0[jb + 1]) ++jb;
  lb = (int)blockIdx.x - J_.blk0[jb];
  return jb;
}

// The job's NV partial sums of this block into work[NV lb + i], then its ticket; true in the LAST block of the job to arrive, whose
// lane 0 then holds the totals (summed in block order: the same bits whatever the arrival order).  Release / acquire as grid_sum.
template <int NV>
__device__ __forceinline__ bool job_sum(double (&val)[NV], double* __restrict__ work, double* ctl, int nb, int lb) {
  __shared__ int is_last;
  double s[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) s[i] = gsum64(val[i]);
  if (threadIdx.x == 0)
    for (int i = 0; i < NV; ++i) work[NV * lb + i] = s[i];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  unsigned int* ticket = reinterpret_cast<unsigned int*>(ctl + C_TICKET);
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    is_last = t == (unsigned int)nb - 1;
    if (is_last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!is_last) return false;
  if (threadIdx.x == 0) {
    for (int i = 0; i < NV; ++i) {
      double tot = 0.0;
      for (int b = 0; b < nb; ++b) tot += work[NV * b + i];
      val[i] = tot;
    }
    *ticket = 0u;                                           // (every block of the job has taken its ticket)
  }
  return true;
}

// ---- the controller's formulas, by value: what ctl_init1 / ctl_init2 / ctl_attempt below do with a job's norms, and kq_paths
// (xw_tdopri_paths.hip) with the norms of a lane's own path ---------------------------------------------------------------------
// torchdiffeq _select_initial_step: h0 from d0 = ||y0 / scale||, d1 = ||f0 / scale||
__device__ __forceinline__ double ctl_h0(double d0, double d1) { return (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1; }
// ... and the first step from d1, d2 = ||(f(t0 + h0, y0 + h0 f0) - f0) / scale|| / h0
// (ctl_init2 keeps its own text of these two lines: routed through this function its kernels compile to other instructions)
__device__ __forceinline__ double ctl_first_dt(double d1, double d2, double h0) {
  const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow(0.01 / fmax(d1, d2), 1.0 / 5);
  return fmin(100 * h0, h1);
}
// torchdiffeq _optimal_step_size, order 5: the step size after an attempt over dt with error ratio `ratio` (not NaN)
__device__ __forceinline__ double ctl_next_dt(double dt, double ratio) {
  if (ratio == 0.0) return dt * DP_IFACTOR;
  const double dfac = ratio < 1.0 ? 1.0 : DP_DFACTOR;
  return dt * fmin(DP_IFACTOR, fmax(DP_SAFETY / pow(ratio, 1.0 / 5), dfac));
}

// ---- the step controller: lane 0 of the last block of a job, with the job's totals ---------------------------------------------
// torchdiffeq _select_initial_step, first half: d0 = ||y0 / scale||, d1 = ||f0 / scale|| (acc: their squared sums), h0
__device__ __forceinline__ void ctl_init1(const double (&acc)[2], int N, int Hn, double* c) {
  const double cnt = (double)N * Hn;
  const double d0 = sqrt(acc[0] / cnt), d1 = sqrt(acc[1] / cnt);
  c[C_H0] = ctl_h0(d0, d1);
  c[C_D1] = d1;
}

// second half: d2 from acc = the squared sum of (f(t0 + h0, y0 + h0 f0) - f0) / scale, the first step; the controller starts
__device__ __forceinline__ void ctl_init2(double acc, int N, int Hn, const double* __restrict__ tf, int L, double* c, double* rec_t) {
  const double t0 = tf[0], h0 = c[C_H0];
  const double d1 = c[C_D1], d2 = sqrt(acc / ((double)N * Hn)) / h0;
  const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow(0.01 / fmax(d1, d2), 1.0 / 5);
  const double dt = fmin(100 * h0, h1);
  const bool done = !(tf[L - 1] > t0);
  c[C_T0] = t0;
  c[C_DT] = dt;
  c[C_NACC] = 0.0;
  c[C_NATT] = 0.0;
  c[C_DONE] = done ? 1.0 : 0.0;
  c[C_STATUS] = 0.0;
  c[C_RATIO] = 0.0;
  c[C_GAP] = HUGE_VAL;
  rec_t[0] = t0;
  if (!done && !(t0 + dt > t0)) {                           // torchdiffeq: assert t0 + dt > t0, 'underflow in dt'
    c[C_STATUS] = XW_DOPRI_UNDERFLOW;
    c[C_DONE] = 1.0;
  }
}

// after an attempt from t0 over dt with na steps accepted so far (torchdiffeq _adaptive_step / _optimal_step_size, order 5):
// acc = the squared sum of the scaled error; room: the record has a slot for the candidate
__device__ __forceinline__ void ctl_attempt(double acc, int N, int Hn, double t0, double dt, int na, bool room, int max_steps,
                                            const double* __restrict__ tf, int L, double* c, double* rec_t, double* rec_h) {
  const double t1 = t0 + dt;
  const double ratio = sqrt(acc / ((double)N * Hn));
  c[C_NATT] += 1.0;
  c[C_RATIO] = ratio;
  c[C_GAP] = fmin(c[C_GAP], fabs(ratio - 1.0));
  if (ratio != ratio) {                                     // NaN: torchdiffeq rejects and its next dt is NaN (the underflow assert)
    c[C_STATUS] = XW_DOPRI_NONFINITE;
    c[C_DONE] = 1.0;
    return;
  }
  const bool accept = ratio <= 1.0;
  const double dtn = ctl_next_dt(dt, ratio);
  double tn = t0;
  if (accept) {
    if (!room) {
      c[C_STATUS] = XW_DOPRI_CAPACITY;
      c[C_DONE] = 1.0;
      return;
    }
    rec_t[na + 1] = t1;
    rec_h[na] = dt;
    c[C_NACC] = (double)(na + 1);
    tn = t1;
  }
  c[C_T0] = tn;
  c[C_DT] = dtn;
  if (!(tf[L - 1] > tn)) {
    c[C_DONE] = 1.0;
  } else if (accept && na + 1 >= max_steps) {
    c[C_STATUS] = XW_DOPRI_STEPS;
    c[C_DONE] = 1.0;
  } else if (!(tn + dtn > tn)) {
    c[C_STATUS] = XW_DOPRI_UNDERFLOW;
    c[C_DONE] = 1.0;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
template <class J> int pack_jobs(const J* jobs, int njobs, Jobs<J>& P) {
  if (!jobs || njobs < 1 || njobs > XW_DOPRI_MAXJOBS) return XW_E_ARG;
  P.njobs = njobs;
  P.blk0[0] = 0;
  for (int i = 0; i < njobs; ++i) P.j[i] = jobs[i];
  return 0;                                                 // (blk0: below, from the job kind's N)
}

// the jobs of a forward launch (init, attempts), paths_per_block paths to a block
inline int fwd_jobs(const XwDopriJob* jobs, int njobs, Jobs<XwDopriJob>& P, int paths_per_block) {
  const int e = pack_jobs(jobs, njobs, P);
  if (e) return e;
  for (int i = 0; i < njobs; ++i) {
    const XwDopriJob& j = jobs[i];
    if (!j.xT || !j.start || !j.u || !j.rec_y || !j.rec_t || !j.rec_h || !j.fbuf || !j.ctl || !j.work || j.N < 1 || j.cap < 0)
      return XW_E_ARG;
    P.blk0[i + 1] = P.blk0[i] + (j.N + paths_per_block - 1) / paths_per_block;
  }
  return 0;
}

// the jobs of a sweep launch: record and job well-formed for `mode`, the slabs (Pu doubles per 16 paths) zeroed with mode bit 1.
// zero_each: a job's slabs as soon as the job has passed, so that a failed memset is reported ahead of a later job's XW_E_ARG
// (xw_dopri5_sweep); else once every job has passed (xw_tdopri5_sweep)
inline int sweep_jobs(const XwDopriSweepJob* jobs, int njobs, Jobs<XwDopriSweepJob>& P, int mode, long Pu, int paths_per_block,
                      bool zero_each, hipStream_t s) {
  const int e = pack_jobs(jobs, njobs, P);
  if (e) return e;
  for (int pass = 0; pass < 2; ++pass)
    for (int i = 0; i < njobs; ++i) {
      const XwDopriSweepJob& j = jobs[i];
      if (pass == 0) {
        if (!j.rec_y || !j.rec_t || !j.rec_h || !j.ctl || !sweep_job_ok(j.b, mode)) return XW_E_ARG;
        P.blk0[i + 1] = P.blk0[i] + (j.b.N + paths_per_block - 1) / paths_per_block;
      }
      if ((mode & 2) && zero_each == (pass == 0)) {
        const hipError_t he = hipMemsetAsync(j.b.gslab, 0, sizeof(double) * Pu * ((j.b.N + 15) / 16), s);
        if (he != hipSuccess) return (int)he;
      }
    }
  return 0;
}
