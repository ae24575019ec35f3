// xw_ode_select.h -- which kernel a launch of the fused stepper lands on: small pure host functions from what a launch asks for to a
// slot of the kernel tables of xw_ode_fwd.h and xw_ode.hip, or an error.  No HIP in here (a plain C++ program can call them);
// tests/stepper_inventory.reaches() restates these rules in Python, in terms of what a caller of kernels.ode_fwd_multi /
// ode_bwd_multi passes.
#pragma once
#include "xnwan.h"

// narrow tiles (xw_ode_n4.h) exist in the 4x4x4 form only: in the wide container a launch that asks for them runs the 16-path kernels
#ifdef XW_ODE_WIDE16
#define XW_ODE_HAS_NARROW 0
#else
#define XW_ODE_HAS_NARROW 1
#endif
// the depths of an object's tables: 1 .. XW_ODE_MAX_LAYERS (xw_common.h), or one depth only in development builds (ISA listings, A/B
// variants: -DXW_ODE_ONLY_M=<m>; the other rows stay empty)
#ifdef XW_ODE_ONLY_M
#define XW_ODE_HAS_DEPTH(M) ((M) == XW_ODE_ONLY_M)
#else
#define XW_ODE_HAS_DEPTH(M) true
#endif

namespace {

constexpr int XW_ODE_DEPTHS = 10;      // (= XW_ODE_MAX_LAYERS of xw_common.h, asserted in xw_ode_core.h)
inline bool depth_compiled(int m) { return m >= 1 && m <= XW_ODE_DEPTHS && XW_ODE_HAS_DEPTH(m); }

// The slots of a table stand in the order in which the kernels of one depth stand in the width's code object (the compiler emits
// them as the table names them).  The order is part of the machine code: in the 4x4x4 form k_ode_bwd_duo reaches its constant
// table xw_duo_const by a pc-relative offset, which is the same from build to build only while the same kernels stand in front of it.

// ---- forward: [n4::k_ode_fwd_n4 x 7 |] k_ode_fwd x 7, <H, K, M, METHOD, ACT> at METHOD * 3 + ACT of its seven (ACT: 0 no activation
// store, 1 the full store, 2 only what an x-only sweep reads; rk4 keeps no store)
constexpr int XW_FWD_KINDS = 7;
constexpr int XW_FWD_SLOTS = XW_FWD_KINDS * (1 + XW_ODE_HAS_NARROW);
struct FwdChoice {
  int rc;          // 0, or XW_E_ARG: a method outside the table
  bool narrow;     // a kernel of the narrow tiles: four waves per 16-path tile
  int slot;
};
inline FwdChoice choose_fwd(int method, bool store, bool x_only, bool narrow_asked) {
  const int kind = method * 3 + (store ? (x_only ? 2 : 1) : 0);
  if (kind < 0 || kind >= XW_FWD_KINDS) return {XW_E_ARG, false, 0};
  const bool narrow = narrow_asked && XW_ODE_HAS_NARROW;
  return {0, narrow, (narrow ? 0 : XW_FWD_KINDS * XW_ODE_HAS_NARROW) + kind};
}

// ---- sweeps from the activation store.  mode: the word of xw_ode_bwd_multi (bit 1 weight gradients, 3 the continuous adjoint, 4 narrow
// tiles); store: every job of the launch brings an activation store.  The slots of a depth (METHOD: euler 0, midpoint 1):
//   4x4x4 form   0, 1  n4::k_ode_bwd_n4<.., METHOD, true>     narrow tiles with weight gradients
//                2, 4  k_ode_bwd_duo<.., METHOD>              SWEEP_DUO: weight gradients, chain wave + partner wave
//                3, 5  k_ode_bwd<.., METHOD, false, true>     SWEEP_STORE: x-only, one wave per tile
//                6, 7  n4::k_ode_bwd_n4<.., METHOD, false>    narrow tiles, x-only
//   wide form    0, 2 the duo sweep, 1, 3 the x-only sweep
//   SWEEP_RECOMP: no slot -- the width's recomputing object (xw_ode_bwd_recomp_w): no store, rk4, the continuous adjoint
enum SweepKind { SWEEP_STORE, SWEEP_DUO, SWEEP_N4, SWEEP_RECOMP };
constexpr int XW_SWEEP_FIRST16 = 2 * XW_ODE_HAS_NARROW;      // first slot of the 16-path kernels
constexpr int XW_SWEEP_SLOTS = 4 + 4 * XW_ODE_HAS_NARROW;
struct SweepChoice {
  int rc;          // 0, or XW_E_ARG
  SweepKind kind;
  int slot;
};
inline SweepChoice choose_sweep(int method, int mode, bool store) {
  const bool params = (mode & 2) != 0, adj = (mode & 8) != 0, narrow = (mode & 16) != 0 && XW_ODE_HAS_NARROW;
  // (a method below 0 -- the public entry points turn it away -- is not euler, and so takes the midpoint slot wherever the ladders
  //  these tables replace asked "euler or not": kept as it was)
  const int m01 = method == 0 ? 0 : 1;
  if (narrow) {
    if (adj || method > 1 || !store) return {XW_E_ARG, SWEEP_N4, 0};
    return {0, SWEEP_N4, (params ? 0 : 6) + m01};
  }
  if (adj || !store || method > 1) return {0, SWEEP_RECOMP, 0};
  if (XW_ODE_HAS_NARROW && method < 0) return {XW_E_ARG, SWEEP_STORE, 0};
  return {0, params ? SWEEP_DUO : SWEEP_STORE, XW_SWEEP_FIRST16 + 2 * m01 + (params ? 0 : 1)};
}
// the recomputing object: k_ode_bwd<H, K, M, METHOD, PARAMS, false, ADJ>, slot = METHOD * 4 + PARAMS * 2 + ADJ; -1: no such method
constexpr int XW_RECOMP_SLOTS = 12;
inline int recomp_slot(int method, bool params, bool adj) {
  return method < 0 || method > 2 ? -1 : method * 4 + (params ? 2 : 0) + (adj ? 1 : 0);
}

// ---- the duo sweep's grid (k_ode_bwd_duo): with exactly two rounds of tiles over the chip's CUs a spacer round of `spread` = ncu blocks
// goes in between (103 against 142 us at 512 tiles; with three rounds the third block of a CU meets the first again either way -- 149
// against 145 us --, and from four rounds on every SIMD hosts two waves whatever the order)
struct DuoGrid {
  int spread, blocks;
};
inline DuoGrid duo_grid(int tiles, int ncu, bool spread_on) {
  const int spread = (spread_on && ncu > 0 && tiles > ncu && tiles <= 2 * ncu) ? ncu : 0;
  const int rounds = spread ? (tiles + ncu - 1) / ncu : 0;
  return {spread, spread ? (2 * (rounds - 1)) * ncu + (tiles - (rounds - 1) * ncu) : tiles};
}

}  // namespace
