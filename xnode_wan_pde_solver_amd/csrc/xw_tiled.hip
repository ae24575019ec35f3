// xw_tiled.hip -- the TILED stepper family: u_theta's forward pass and its reverse sweep at the network's own runtime widths,
// u_hidden_dim H <= 256, u_hidden_hidden_dim K <= 256, u_layers 1..32, fixed-grid euler / midpoint / rk4 (3/8 rule).
//
// The fused kernels of xw_ode_fwd.h / xw_ode.hip keep a path tile's state and the field's weights in registers, sized at compile time, and stop
// at (64, 16); the generic path (xw_generic.hip) runs one path per lane on the vector ALU and stops at the same widths.  Here
// one wave owns a tile of 16 paths for every step of a job and runs every layer of the field as a [K_out x K_in] . [K_in x 16]
// product on v_mfma_f64_16x16x4 (xw_common.h: "chain layout", features on the rows, the 16 paths on the columns), the widths
// padded to multiples of 4 / 16 inside the kernel only.  Weights stream from global memory through L2 (at (128, 64, 8) the
// field is ~46 k doubles, more than the LDS holds).  The tile's vectors -- state, stage inputs, layer activations -- live in a
// per-tile slice of a caller-provided workspace (xw_tiled_ode_work), [rows][16] with the path innermost, so every phase
// reads and writes whole 512-byte rows; the wave is its own workgroup and orders its phases with a barrier.
//
// The sweep recomputes each step's stages from the checkpoints Y (fixed grid: the steps are the sample times) and takes the
// vector-Jacobian products; weight gradients are outer products over the tile's 16 paths on the same instruction (the paths are
// its reduction dimension), added to the tile's slab of gslab[(N + 15) / 16][P_u] -- today's slab format, so k_slab_sum, the
// all-reduce and Adam are unchanged.  Every slab entry is updated by one fixed lane of one wave in program order: no float
// atomics, the same bits on every run and in a captured graph.  Lanes of a tile past the end of a job walk along with the last
// path on a zero cotangent: they add exact zeros and store nothing.
//
// Parameters are read in the generic path's blob layout (u_offsets(d, H, K) at the network's own widths).
// Not here: the continuous adjoint (mode bit 3), narrow tiles (mode bit 4), an activation store -- XW_E_DIMS.
#include "xw_common.h"
#include "xnwan.h"

namespace {
#include "xw_generic_cot.h"
#include "xw_tiled_blocks.h"

// ---- solver 'explicit_adams' (torchdiffeq fixed_adams.py AdamsBashforth): the history of field values ----------------------
// For step n = 0 .. L-2: f_n = F(t_n, y_n) joins the history (most recent first, at most XWA_HIST entries); steps 0 and 1 are
// rk4 steps (3/8 rule) with k1 = f_n, step n >= 2 is y_{n+1} = y_n + sum_{j < ord_n} (dt_n beta[ord_n][j]) f_{n-j} with
// ord_n = min(n + 1, XWA_HIST) -- the fixed coefficients at the current dt, also on a non-uniform grid.
#define XWA_HIST 11                                   // torchdiffeq: deque(maxlen = _MAX_ORDER - 1), _MAX_ORDER = 12

// beta[k][j]: the k-step Adams-Bashforth row, most recent value first -- the integral over [0, 1] of the Lagrange basis
// polynomial of node -j among the nodes 0, -1, .., -(k-1) (in steps).  Derived in exact integer arithmetic: the basis numerator
// prod_{i != j} (s + i) has integer coefficients c_p, its integral is sum_p c_p / (p + 1) = num / 27720 (27720 = lcm(1 .. 11)),
// the denominator is (-1)^j j! (k-1-j)!.  num and 27720 j! (k-1-j)! are below 2^53, so one division gives the correctly
// rounded value -- the same double as float(Fraction(num, den)).
struct AbRows { double b[XWA_HIST + 1][XWA_HIST]; };
__host__ __device__ constexpr AbRows ab_rows() {
  AbRows r{};
  for (int k = 1; k <= XWA_HIST; ++k)
    for (int j = 0; j < k; ++j) {
      long long c[XWA_HIST + 1] = {1};               // coefficients of prod_{i != j, i < k} (s + i), lowest power first
      int deg = 0;
      for (int i = 0; i < k; ++i) {
        if (i == j) continue;
        for (int p = deg + 1; p >= 1; --p) c[p] = c[p - 1] + (long long)i * c[p];
        c[0] *= i;
        ++deg;
      }
      long long num = 0, den = 27720;
      for (int p = 0; p <= deg; ++p) num += c[p] * (27720 / (p + 1));
      for (int i = 2; i <= j; ++i) den *= i;
      for (int i = 2; i <= k - 1 - j; ++i) den *= i;
      r.b[k][j] = (double)((j & 1) ? -num : num) / (double)den;
    }
  return r;
}
__constant__ AbRows kAB = ab_rows();
constexpr AbRows kABhost = ab_rows();

__device__ __forceinline__ int ab_order(int n) { return n + 1 < XWA_HIST ? n + 1 : XWA_HIST; }

__global__ void __launch_bounds__(64) kt_ode_fwd(XwOdeFwdJob job, const double* __restrict__ tf, const double* __restrict__ theta,
                                                  int method, int L, int d, int H, int K, int m, double* __restrict__ work) {
  set_prio(job.prio_drop);
  const int N = job.N, p0 = blockIdx.x * 16;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TileWork w = tile_work(0, d, H, K, m);
  double* ws = work + (long)blockIdx.x * w.total;
  double* y = ws + w.hv;
  double* acc = y + 16L * H;
  double* cc = acc + 16L * H;
  double* tmp = cc + 16L * H;
  double* fo = tmp + 16L * H;
  double* st = ws + w.st;
  const int l16 = lane_id() & 15;
  if (lane_id() < 16) st[l16] = job.start[p0 + l16 < N ? p0 + l16 : N - 1];
  tile_x(n, w, ws, job.xT, N, p0);
  tlift(n, st, acc, cc, y);
  for (int l = 0; l < L; ++l) {
    if (l > 0) tstep_fwd(n, w, ws, method, tf[l - 1], tf[l] - tf[l - 1], y, acc, cc, tmp, fo);
    tput_output(n, job.u, job.Y, l, N, p0, y);
  }
}

// the explicit_adams forward pass: kt_ode_fwd with the field values f_n kept in a ring of XWA_HIST H-vectors behind the tile's
// TileWork (slot n % XWA_HIST); step n >= 2 is one field evaluation and the Adams-Bashforth sum, steps 0 and 1 are the rk4 step
// of kt_ode_fwd (tstep_rk4) from k1 = f_n
__global__ void __launch_bounds__(64) kt_adams_fwd(XwOdeFwdJob job, const double* __restrict__ tf, const double* __restrict__ theta,
                                                   int L, int d, int H, int K, int m, double* __restrict__ work) {
  set_prio(job.prio_drop);
  const int N = job.N, p0 = blockIdx.x * 16;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TileWork w = tile_work(0, d, H, K, m);
  double* ws = work + (long)blockIdx.x * (w.total + 16L * H * XWA_HIST);
  double* y = ws + w.hv;
  double* acc = y + 16L * H;
  double* cc = acc + 16L * H;
  double* tmp = cc + 16L * H;
  double* fo = tmp + 16L * H;
  double* ring = ws + w.total;
  double* st = ws + w.st;
  const int l16 = lane_id() & 15;
  if (lane_id() < 16) st[l16] = job.start[p0 + l16 < N ? p0 + l16 : N - 1];
  tile_x(n, w, ws, job.xT, N, p0);
  tlift(n, st, acc, cc, y);
  for (int l = 0; l < L; ++l) {
    if (l > 0) {
      const int s = l - 1;                                       // the step y_s -> y_l
      const double t0 = tf[s], dt = tf[l] - tf[s];
      double* k1 = ring + 16L * H * (s % XWA_HIST);
      tfield(n, w, ws, t0, y, k1, false);                        // f_s joins the history
      if (s >= 2) {
        const int ord = ab_order(s);
        for (int e = lane_id(); e < 16 * H; e += 64) {
          double dy = 0.0;
          for (int j = 0; j < ord; ++j) dy = fma(dt * kAB.b[ord][j], ring[16L * H * ((s - j) % XWA_HIST) + e], dy);
          y[e] += dy;
        }
        sync_tile();
      } else {                                                   // rk4 start-up step from k1 = f_s
        tstep_rk4(n, w, ws, t0, dt, y, k1, acc, cc, tmp, fo);
      }
    }
    tput_output(n, job.u, job.Y, l, N, p0, y);
  }
}

// The fixed-grid sweep keeps its own text -- step reverses, cotangent block and tail written out, none of the shared sweep pieces of
// xw_tiled_blocks.h (tstep_rk4_bwd, tcot_output, sweep_prologue, sweep_tail), which kt_adams_bwd and the dopri5 sweep use: with any
// of them inlined here the compiler lays this kernel and the out-of-line blocks out differently and midpoint's sweep at (20, 10, 8)
// measured 6 to 11 % slower (profiles/r18_tiled_shared_blocks.md).  A change to the tail or to the rk4 reverse lands here AND there;
// tests/test_gpu_adams.py pins the two to the same bits.
__global__ void __launch_bounds__(64) kt_ode_bwd(XwOdeBwdJob job, const double* __restrict__ tf, const double* __restrict__ theta,
                                                  int method, int L, int d, int H, int K, int m, int mode, double* __restrict__ work) {
  set_prio(mode >> 5);
  const int N = job.N, p0 = blockIdx.x * 16;
  const bool want_x = (mode & 1) != 0, ones_x = (mode & 4) != 0;
  double* slab = (mode & 2) ? job.gslab + (long)blockIdx.x * u_offsets(d, H, K).total : nullptr;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TileWork w = tile_work(1, d, H, K, m);
  double* ws = work + (long)blockIdx.x * w.total;
  double* hv = ws + w.hv;
  double* lam = hv;
  double* Y1 = hv + 16L * H * 1;
  double* Y2 = hv + 16L * H * 2;
  double* Y3 = hv + 16L * H * 3;
  double* Y4 = hv + 16L * H * 4;
  double* cc = hv + 16L * H * 5;
  double* fo = hv + 16L * H * 6;
  double* g4 = hv + 16L * H * 7;
  double* g3 = hv + 16L * H * 8;
  double* g2 = hv + 16L * H * 9;
  double* a = hv + 16L * H * 10;
  double* gy = hv + 16L * H * 11;
  double* ub = ws + w.ub;
  double* st = ws + w.st;
  double* Sx = ws + w.total - 16L * K;
  const int l16 = lane_id() & 15;
  const bool lane_active = p0 + l16 < N;
  if (lane_id() < 16) st[l16] = job.start[lane_active ? p0 + l16 : N - 1];
  for (int e = lane_id(); e < 16 * K; e += 64) Sx[e] = 0.0;
  for (int e = lane_id(); e < 16 * H; e += 64) lam[e] = 0.0;
  tile_x(n, w, ws, job.xT, N, p0);
  const double* flw = theta + n.o.FLw;
  for (int l = L - 1; l >= 1; --l) {
    if (lane_id() < 16) ub[l16] = lane_active ? cot_u(job, l, L, p0 + l16) : 0.0;
    for (int e = lane_id(); e < 16 * H; e += 64) {
      const int p = p0 + (e & 15);
      Y1[e] = job.Y[((long)(l - 1) * H + (e >> 4)) * N + (p < N ? p : N - 1)];
      Y2[e] = job.Y[((long)l * H + (e >> 4)) * N + (p < N ? p : N - 1)];      // (y_l, for the read-out's gradient)
    }
    sync_tile();
    for (int e = lane_id(); e < 16 * H; e += 64) lam[e] = fma(flw[e >> 4], ub[e & 15], lam[e]);
    if (slab) {
      trowsum(slab, n.o.FLw, 1, H, Y2, ub, 1.0);
      if (lane_id() == 0) {
        double s = 0.0;
        for (int p = 0; p < 16; ++p) s += ub[p];
        slab[n.o.FLb] += s;
      }
    }
    sync_tile();
    // y_l = step(y_{l-1}): lam becomes the cotangent of y_{l-1}
    const double t0 = tf[l - 1], dt = tf[l] - tf[l - 1];
    if (method == 0) {
      tcomb(H, a, nullptr, dt, lam);
      tfield_vjp(n, w, ws, t0, Y1, a, gy, slab);
      tcomb(H, lam, lam, 1.0, gy);
    } else if (method == 1) {
      tfield(n, w, ws, t0, Y1, fo, true);
      tcomb(H, Y2, Y1, dt / 2, fo);
      tcomb(H, a, nullptr, dt, lam);
      tfield_vjp(n, w, ws, t0 + dt / 2, Y2, a, gy, slab);
      tcomb(H, lam, lam, 1.0, gy);
      tcomb(H, a, nullptr, dt / 2, gy);
      tfield_vjp(n, w, ws, t0, Y1, a, gy, slab);
      tcomb(H, lam, lam, 1.0, gy);
    } else {
      tfield(n, w, ws, t0, Y1, fo, true);                        // k1; cc = k1
      tcomb(H, cc, nullptr, 1.0, fo);
      tcomb(H, Y2, Y1, dt / 3, fo);
      tfield(n, w, ws, t0 + dt / 3, Y2, fo, true);               // k2
      tcomb(H, Y3, Y1, dt, fo, -dt / 3, cc);
      tcomb(H, cc, cc, -1.0, fo);                                // cc = k1 - k2
      tfield(n, w, ws, t0 + 2 * dt / 3, Y3, fo, true);           // k3
      tcomb(H, Y4, Y1, dt, cc, dt, fo);
      tcomb(H, a, nullptr, dt / 8, lam);
      tfield_vjp(n, w, ws, t0 + dt, Y4, a, g4, slab);
      tcomb(H, a, nullptr, 3 * dt / 8, lam, dt, g4);
      tfield_vjp(n, w, ws, t0 + 2 * dt / 3, Y3, a, g3, slab);
      tcomb(H, a, nullptr, 3 * dt / 8, lam, -dt, g4, dt, g3);
      tfield_vjp(n, w, ws, t0 + dt / 3, Y2, a, g2, slab);
      for (int e = lane_id(); e < 16 * H; e += 64) a[e] = (dt / 8) * lam[e] + dt * g4[e] - (dt / 3) * g3[e] + (dt / 3) * g2[e];
      sync_tile();
      tfield_vjp(n, w, ws, t0, Y1, a, gy, slab);
      for (int e = lane_id(); e < 16 * H; e += 64) lam[e] += g4[e] + g3[e] + g2[e] + gy[e];
      sync_tile();
    }
  }
  // l = 0: read-out, then the lift 1 -> H -> H -> H; with mode bit 2 the x-side outputs are those of the ALL-ONES cotangent
  // while the parameter gradients use the job's own (xw_generic.hip kg_ode_bwd) -- sweep_tail's text
  if (lane_id() < 16) ub[l16] = lane_active ? cot_u(job, 0, L, p0 + l16) : 0.0;
  sync_tile();
  double* p0v = Y2;
  double* p2v = Y3;
  double* y0 = Y4;
  double* l0 = cc;
  double* dh2 = fo;
  double* dh1 = g4;
  tlift(n, st, p0v, p2v, y0);
  if (slab) {
    trowsum(slab, n.o.FLw, 1, H, y0, ub, 1.0);
    if (lane_id() == 0) {
      double s = 0.0;
      for (int p = 0; p < 16; ++p) s += ub[p];
      slab[n.o.FLb] += s;
    }
  }
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 0 && !slab) continue;
    if (pass == 1 && !(want_x && job.gs != nullptr)) continue;
    const bool ones = pass == 1 && ones_x;
    for (int e = lane_id(); e < 16 * H; e += 64) l0[e] = fma(flw[e >> 4], ones ? 1.0 : ub[e & 15], lam[e]);
    sync_tile();
    tgemm(theta + n.o.IL4w, 1, H, H, H, l0, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p2v, dh2);
    tgemm(theta + n.o.IL2w, 1, H, H, H, dh2, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_GATE, p0v, dh1);
    if (pass == 0) {
      touter(slab, n.o.IL4w, H, H, H, l0, p2v, A_RELU);
      touter(slab, n.o.IL2w, H, H, H, dh2, p0v, A_RELU);
      trowsum(slab, n.o.IL4b, 1, H, l0, nullptr, 1.0);
      trowsum(slab, n.o.IL2b, 1, H, dh2, nullptr, 1.0);
      trowsum(slab, n.o.IL0w, 1, H, dh1, st, 1.0);
      trowsum(slab, n.o.IL0b, 1, H, dh1, nullptr, 1.0);
      sync_tile();
    } else if (lane_id() < 16 && lane_active) {
      double s = 0.0;
      for (int i = 0; i < H; ++i) s = fma(theta[n.o.IL0w + i], dh1[i * 16 + l16], s);
      job.gs[p0 + l16] = s;
    }
  }
  // the x columns and the bias of the input layer, from the summed cotangent of its pre-activation
  if (slab) {
    trowsum(slab, n.o.Winb, 1, K, Sx, nullptr, 1.0);
    touter(slab, n.o.Win, n.o.ldin, K, d, Sx, ws + w.xt, A_PLAIN);
  }
  if (want_x && job.gx != nullptr) {
    double* gxt = ws + w.xt + 16L * d;
    tgemm(theta + n.o.Win, 1, n.o.ldin, d, K, Sx, A_PLAIN, nullptr, nullptr, 0, 0.0, nullptr, E_NONE, nullptr, gxt);
    for (int e = lane_id(); e < 16 * d; e += 64)
      if (p0 + (e & 15) < N) job.gx[(long)(e >> 4) * N + p0 + (e & 15)] = gxt[e];
  }
}

// the explicit_adams sweep: kt_ode_bwd's rk4 sweep (method 2) with the history terms.  Behind the tile's TileWork: a ring of the
// XWA_HIST last finished cotangents ybar_l (slot l % XWA_HIST) and fbar, the cotangent of the history entry f_k,
//   fbar_k = sum_{n = max(k, 2)}^{min(k + XWA_HIST - 1, L - 2)} dt_n beta[ord_n][n - k] ybar_{n+1}      (dt_n constants);
// then ybar_k = ybar_{k+1} + J_F(t_k, y_k)^T fbar_k (+ the cotangent on u at k) for k >= 2, with the field's activations recomputed
// from Y[k].  The start-up steps k = 0, 1 take the rk4 reverse with fbar_k added to the cotangent of k1 (the same evaluation as
// the history entry): tstep_rk4_bwd with fbar_k as the further cotangent on k1.
__global__ void __launch_bounds__(64) kt_adams_bwd(XwOdeBwdJob job, const double* __restrict__ tf, const double* __restrict__ theta,
                                                   int L, int d, int H, int K, int m, int mode, double* __restrict__ work) {
  set_prio(mode >> 5);
  const int N = job.N, p0 = blockIdx.x * 16;
  double* slab = (mode & 2) ? job.gslab + (long)blockIdx.x * u_offsets(d, H, K).total : nullptr;
  const Net n = {theta, u_offsets(d, H, K), d, H, K, m};
  const TileWork w = tile_work(1, d, H, K, m);
  double* ws = work + (long)blockIdx.x * (w.total + 16L * H * (XWA_HIST + 1));
  const SweepVecs v = sweep_vecs(ws + w.hv, H);
  double* ring = ws + w.total;
  double* fb = ring + 16L * H * XWA_HIST;
  sweep_prologue(n, w, ws, job, p0, v.lam);
  for (int l = L - 1; l >= 1; --l) {
    tload(H, N, p0, job.Y + (long)(l - 1) * H * N, v.Y1);
    tload(H, N, p0, job.Y + (long)l * H * N, v.Y2);
    tcot_output(job, n, l, L, p0, ws + w.ub, v.Y2, v.lam, slab);
    double* rl = ring + 16L * H * (l % XWA_HIST);
    for (int e = lane_id(); e < 16 * H; e += 64) rl[e] = v.lam[e];   // ybar_l is complete: into the ring
    const int k = l - 1;
    const double t0 = tf[k], dt = tf[l] - tf[k];
    const int q0 = k > 2 ? k : 2, q1 = k + XWA_HIST - 1 < L - 2 ? k + XWA_HIST - 1 : L - 2;
    for (int e = lane_id(); e < 16 * H; e += 64) {
      double s = 0.0;
      for (int q = q0; q <= q1; ++q) s = fma((tf[q + 1] - tf[q]) * kAB.b[ab_order(q)][q - k], ring[16L * H * ((q + 1) % XWA_HIST) + e], s);
      fb[e] = s;
    }
    sync_tile();
    if (k >= 2) {                                                  // y_l = y_k + sum_j c_j f_{k-j}: lam becomes ybar_k
      tfield_vjp(n, w, ws, t0, v.Y1, fb, v.gy, slab);
      tcomb(H, v.lam, v.lam, 1.0, v.gy);
    } else {                                                       // rk4 start-up step; + fbar_k: k1 is f_k
      tstep_rk4_bwd(n, w, ws, t0, dt, v, slab, fb);
    }
  }
  sweep_tail(n, w, ws, job, L, p0, mode, slab, v.lam, v.Y2, v.Y3, v.Y4, v.cc, v.fo, v.g4);
}

}  // namespace

// ---- entry points (include/xnwan.h) -------------------------------------------------------------------------------------------
extern "C" int xw_tiled_ode_ok(int d, int H, int K, int m) {
  return H >= 1 && H <= XWT_MAX_H && K >= 1 && K <= XWT_MAX_K && m >= 1 && m <= XWT_MAX_M && d >= 1 && d + 2 <= 128;
}

// doubles of workspace per tile: the TileWork, and for explicit_adams the history ring (+ fbar in the sweep) behind it
static long tile_stride(bool ab, int sweep, int d, int H, int K, int m) {
  return tile_work(sweep != 0, d, H, K, m).total + (ab ? 16L * H * (XWA_HIST + (sweep ? 1 : 0)) : 0);
}

extern "C" int xw_tiled_ode_work(int sweep, int d, int H, int K, int m) {
  if (!xw_tiled_ode_ok(d, H, K, m)) return XW_E_DIMS;
  return (int)tile_work(sweep != 0, d, H, K, m).total;
}

extern "C" int xw_tiled_ode_bwd_slabs(int N) { return (N + 15) / 16; }

static int check_common(int njobs, const double* t, const double* theta, int method, int L, int d, int H, int K, int m,
                        const double* work) {
  if (njobs < 1 || !t || !theta || !work || L < 1 || method < 0 || method > 2) return XW_E_ARG;
  if (!xw_tiled_ode_ok(d, H, K, m)) return XW_E_DIMS;
  return 0;
}

static int tiled_fwd(bool ab, const XwOdeFwdJob* jobs, int njobs, const double* t, const double* theta, int method, int L, int d,
                     int H, int K, int m, double* zero16, double* work, void* stream) {
  if (!jobs) return XW_E_ARG;
  const int c = check_common(njobs, t, theta, method, L, d, H, K, m, work);
  if (c) return c;
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < njobs; ++i)
    if (!jobs[i].xT || !jobs[i].start || !jobs[i].u || jobs[i].N < 1) return XW_E_ARG;
  if (zero16 != nullptr) {
    const hipError_t e = hipMemsetAsync(zero16, 0, 16 * sizeof(double), s);
    if (e != hipSuccess) return (int)e;
  }
  const long per = tile_stride(ab, 0, d, H, K, m);
  long off = 0;
  for (int i = 0; i < njobs; ++i) {
    const int tiles = (jobs[i].N + 15) / 16;
    if (ab) hipLaunchKernelGGL(kt_adams_fwd, dim3(tiles), dim3(64), 0, s, jobs[i], t, theta, L, d, H, K, m, work + off);
    else hipLaunchKernelGGL(kt_ode_fwd, dim3(tiles), dim3(64), 0, s, jobs[i], t, theta, method, L, d, H, K, m, work + off);
    off += per * tiles;
  }
  return xw_launch_status();
}

static int tiled_bwd(bool ab, const XwOdeBwdJob* jobs, int njobs, const double* t, const double* theta, int method, int L, int d,
                     int H, int K, int m, int mode, double* work, void* stream) {
  if (!jobs || (mode & 3) == 0) return XW_E_ARG;
  const int c = check_common(njobs, t, theta, method, L, d, H, K, m, work);
  if (c) return c;
  if (mode & (8 | 16)) return XW_E_DIMS;                  // (no continuous adjoint, no narrow tiles in this family)
  if ((mode & 4) && (mode & 3) != 3) return XW_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long P = u_offsets(d, H, K).total;
  for (int i = 0; i < njobs; ++i)
    if (!jobs[i].Y || !sweep_job_ok(jobs[i], mode)) return XW_E_ARG;
  const long per = tile_stride(ab, 1, d, H, K, m);
  long off = 0;
  for (int i = 0; i < njobs; ++i) {
    const XwOdeBwdJob& j = jobs[i];
    const int tiles = (j.N + 15) / 16;
    if (mode & 2) {
      const hipError_t e = hipMemsetAsync(j.gslab, 0, sizeof(double) * P * tiles, s);
      if (e != hipSuccess) return (int)e;
    }
    if (ab) hipLaunchKernelGGL(kt_adams_bwd, dim3(tiles), dim3(64), 0, s, j, t, theta, L, d, H, K, m, mode, work + off);
    else hipLaunchKernelGGL(kt_ode_bwd, dim3(tiles), dim3(64), 0, s, j, t, theta, method, L, d, H, K, m, mode, work + off);
    off += per * tiles;
  }
  return xw_launch_status();
}

extern "C" int xw_tiled_ode_fwd_multi(const XwOdeFwdJob* jobs, int njobs, const double* t, const double* theta, int method, int L,
                                      int d, int H, int K, int m, double* zero16, double* work, void* stream) {
  return tiled_fwd(false, jobs, njobs, t, theta, method, L, d, H, K, m, zero16, work, stream);
}

extern "C" int xw_tiled_ode_bwd_multi(const XwOdeBwdJob* jobs, int njobs, const double* t, const double* theta, int method, int L,
                                      int d, int H, int K, int m, int mode, double* work, void* stream) {
  return tiled_bwd(false, jobs, njobs, t, theta, method, L, d, H, K, m, mode, work, stream);
}

// ---- solver 'explicit_adams' on the tiled family --------------------------------------------------------------------------
extern "C" int xw_adams_coef(int k, double* out) {
  if (k < 1 || k > XWA_HIST || !out) return XW_E_ARG;
  for (int j = 0; j < k; ++j) out[j] = kABhost.b[k][j];
  return 0;
}

extern "C" int xw_adams_tiled_work(int sweep, int d, int H, int K, int m) {
  if (!xw_tiled_ode_ok(d, H, K, m)) return XW_E_DIMS;
  return (int)tile_stride(true, sweep, d, H, K, m);
}

extern "C" int xw_adams_tiled_fwd_multi(const XwOdeFwdJob* jobs, int njobs, const double* t, const double* theta, int L, int d, int H,
                                        int K, int m, double* zero16, double* work, void* stream) {
  return tiled_fwd(true, jobs, njobs, t, theta, 2, L, d, H, K, m, zero16, work, stream);
}

extern "C" int xw_adams_tiled_bwd_multi(const XwOdeBwdJob* jobs, int njobs, const double* t, const double* theta, int L, int d, int H,
                                        int K, int m, int mode, double* work, void* stream) {
  return tiled_bwd(true, jobs, njobs, t, theta, 2, L, d, H, K, m, mode, work, stream);
}
