// check_bwd.hip -- xw_disc_bwd as the library has it (xw_disc_bwd.hip, included below) against rec_select and the recomputing
// kernel's table evaluated directly; check_fwd.hip says how, check.hip holds main().  The record path ends in xw_disc_rec_launch, a
// recorder here (xw_disc_rec.hip is not linked): the key (W, ng, tsum), the slab count and every argument are compared.
#include "recorder.h"
#include "xw_disc_bwd.hip"

int xwg_disc_bwd(const double* xT, const double* t, const double* tpp, const double* phi, const double* vbar, int N, int L, int d, int W,
                 int q, const double* act, double* gslab, int nslab, void* stream) {
  take(shot(SHOT_GENERIC, nullptr, 0, 0, xT, t, tpp, phi, vbar, N, L, d, W, q, act, gslab, nslab, stream));
  return 0;
}
int xw_disc_rec_launch(int W, int ng, bool tsum, int blocks, const double* xT, const double* t, const double* tpp, const double* phi,
                       const double* vbar, int N, int L, int d, double* gslab, const double* act, int q, void* stream) {
  take(shot(SHOT_REC, nullptr, 0, 0, W, ng, (int)tsum, blocks, xT, t, tpp, phi, vbar, N, L, d, gslab, act, q, stream));
  return 0;
}

static Tally check_bwd(int tsum_sw, bool wrong) {
  Tally T = {};
  static double buf[8];
  const double *xT = buf, *t = buf + 1, *tpp = buf + 2, *phi = buf + 3, *vbar = buf + 4, *act_ = buf + 5;
  double* gslab = buf + 6;
  const int widths[] = {50, 64, 96, 128, 40, 127};
  const int depths[] = {0, 8, 9, 10, 17};
  const int paths[] = {1, 17, 63, 64, 65, 128, 192, 32768, 32832, 32833};
  const bool tsum_on = (tsum_sw != 0) != wrong;
  for (int W : widths)
    for (int rec = 0; rec < 2; ++rec)
      for (int q : depths)
        for (int N : paths)
          for (int mode = 0; mode < 3; ++mode)              // path L = 1, path L = 3, point
            for (int d = 1; d <= 126; ++d) {
              const int L = mode == 1 ? 3 : 1;
              const double *tt = mode == 2 ? nullptr : t, *tp = mode == 2 ? tpp : nullptr, *act = rec ? act_ : nullptr;
              g_shots = 0; memset(&g_shot, 0, sizeof(Shot));
              const int rc = xw_disc_bwd(xT, tt, tp, phi, vbar, N, L, d, W, q, act, gslab, nullptr);
              const int blocks = bwd_blocks((long)N * L);
              Shot want;
              int rc_want = 0;
              memset(&want, 0, sizeof(want));
              if (!disc_width_ok(W)) {
                want = shot(SHOT_GENERIC, nullptr, 0, 0, xT, tt, tp, phi, vbar, N, L, d, W, q, act, gslab, blocks, (void*)nullptr);
              } else if (!rec && (q != 9 || W != 50)) {
                rc_want = XW_E_DIMS;                        // (no recomputing kernel away from the reference's shape)
              } else if (rec) {
                const RecKey k = rec_select(N, d, mode == 2, tsum_on);
                want = shot(SHOT_REC, nullptr, 0, 0, W, k.ng, (int)k.tsum, blocks, xT, tt, tp, phi, vbar, N, L, d, gslab, act, q, (void*)nullptr);
              } else {
                want = shot(SHOT_KERNEL, (const void*)bwd_table[d + 2 <= 64 ? 0 : 1][0], (unsigned)blocks, 256u, xT, tt, tp, phi, vbar, N, L, d, gslab, (double*)nullptr, (double*)nullptr);
              }
              char detail[128];
              snprintf(detail, sizeof(detail), "W=%d rec=%d q=%d N=%d L=%d mode=%d d=%d", W, rec, q, N, L, mode, d);
              tally(T, "bwd", rc, rc_want, want, detail);
            }
  return T;
}
