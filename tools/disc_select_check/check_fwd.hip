// check_fwd.hip -- xw_disc_fwd / xw_disc_fwd_xproj as the library has them (xw_disc_fwd.hip, included below) against fwd_select and
// fwd_kernel evaluated directly, under every setting of the library switches (xw_switches.hip, linked in; set between the calls of
// ONE process).  Per call: return code, number of launches, kernel, grid, block, every kernel argument -- the ticket-queue slot
// included --, or what the generic stand-in received.  Host code only; included by check.hip, which holds main().
#include "recorder.h"

#include "xw_disc_fwd.hip"

// the generic path's entry points as recorders (xw_generic.hip is not linked)
int xwg_disc_ok(int, int W, int q) { return W >= 1 && W <= XWG_MAX_W && q >= 0; }
int xwg_disc_fwd(const double* xT, const double* t, const double* tpp, const double* phi, int N, int L, int d, int W, int q, double* v,
                 double* vt, double* gxv, double* gtv, int ngrad, double* act, void* stream) {
  take(shot(SHOT_GENERIC, nullptr, 0, 0, xT, t, tpp, phi, N, L, d, W, q, v, vt, gxv, gtv, ngrad, act, stream));
  return 0;
}

static double buf[8];
static Tally check_fwd(const XwSwitches& sw, bool wrong) {
  Tally T = {};
  static unsigned int slots[2];                 // the wrapper's own counters, mirrored: one per kind of launch, never reset
  const int widths[] = {50, 64, 96, 128, 40, 127};
  const long tiles[] = {1, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4100};
  const int below[] = {0, 1, 15, 48};
  const int caps[] = {0, 1, 255, 256, 257, 511, 512, 513, 3000, -1};
  double *xT = buf, *t = buf + 1, *tpp = buf + 2, *phi = buf + 3, *v = buf + 4, *vt = buf + 5, *gx = buf + 6, *gt = buf + 7;
  static double act_[1], table_[1];
  // (the switches as the expectation takes them; --wrong inverts them, and the run must then report disagreements)
  const bool dyn_on = (sw.disc_dynamic != 0) != wrong, vin_on = (sw.disc_vin_lds != 0) != wrong;
  for (int W : widths)
    for (int rec = 0; rec < 2; ++rec)
      for (long nt : tiles)
        for (int bl : below)
          for (int cap : caps)
            for (int d = 1; d <= 126; ++d)
              for (int form = 0; form < 12; ++form) {       // mode (path L = 1, path L = 3, point) x table x fused gradient
                const int mode = form % 3, table = (form / 3) % 2, grad = form / 6;
                if (table && mode == 2) continue;           // (a table in point mode is refused: not a selection)
                const int L = mode == 1 ? 3 : 1;
                const long P = nt * 16 - bl;
                if (P < 1 || P % L) continue;
                const int N = (int)(P / L), q = grad ? 9 : (d % 2 ? 0 : 16), ngrad = grad ? (N < 17 ? N : 17) : 0;
                double* act = rec ? act_ : nullptr;
                const double* xproj = table ? table_ : nullptr;
                g_capturing = (d / 7) % 2;
                g_shots = 0; memset(&g_shot, 0, sizeof(Shot));
                const int rc = table || (d % 3) ? xw_disc_fwd_xproj(xT, mode == 2 ? nullptr : t, mode == 2 ? tpp : nullptr, phi, N, L, d, W, q, v, vt, grad ? gx : nullptr, grad ? gt : nullptr, ngrad, cap, act, xproj, nullptr)
                                                : xw_disc_fwd(xT, mode == 2 ? nullptr : t, mode == 2 ? tpp : nullptr, phi, N, L, d, W, q, v, vt, grad ? gx : nullptr, grad ? gt : nullptr, ngrad, cap, act, nullptr);
                Shot want;
                if (!disc_width_ok(W)) {
                  want = shot(SHOT_GENERIC, nullptr, 0, 0, (const double*)xT, (const double*)(mode == 2 ? nullptr : t), (const double*)(mode == 2 ? tpp : nullptr), (const double*)phi, N, L, d, W, q, v, vt, grad ? gx : nullptr, grad ? gt : nullptr, ngrad, act, (void*)nullptr);
                } else {
                  const FwdKey k = fwd_select(W, (P + 15) / 16, d, cap, table != 0, dyn_on, vin_on);
                  unsigned int* queue = nullptr;
                  if (k.dyn) {                                   // every ticketed launch draws the next slot of its half
                    const int half = g_capturing ? 1 : 0;
                    const unsigned slot = half * (XW_DISC_SLOTS / 2) + slots[half]++ % (XW_DISC_SLOTS / 2);
                    queue = g_fake_queue + (size_t)slot * ((XW_DISC_NQ + 1) * XW_DISC_QSTRIDE);
                  }
                  want = shot(SHOT_KERNEL, (const void*)fwd_kernel(W, k.vks, rec != 0, k.dyn), (unsigned)k.blocks, 256u, (const double*)xT, (const double*)(mode == 2 ? nullptr : t), (const double*)(mode == 2 ? tpp : nullptr), (const double*)phi, N, L, d, q, v, vt, grad ? gx : nullptr, grad ? gt : nullptr, ngrad, act, queue, xproj);
                }
                char detail[160];
                snprintf(detail, sizeof(detail), "W=%d rec=%d tiles=%ld P=%ld cap=%d d=%d mode=%d table=%d grad=%d", W, rec, nt, P, cap, d, mode, table, grad);
                tally(T, "fwd", rc, 0, want, detail);
              }
  return T;
}
