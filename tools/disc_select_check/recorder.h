// recorder.h -- what check_fwd.hip and check_bwd.hip put in front of the library source they include: the kernel launch as a recorder
// and the few HIP calls of the launch wrappers as constants, so that the program links without the HIP runtime and needs no GPU.
#pragma once
#include <cstdio>
#include <cstring>
#include <set>
#include "xw_common.h"
#include "xnwan.h"

// one call as it left the wrapper: a kernel launch (k the host stub), or a call of a stand-in (k null, `what` says which)
struct Shot {
  const void* k;
  int what, nargs;
  unsigned grid, block;
  unsigned long long a[20];        // every argument, widened to 64 bits
  bool operator==(const Shot& o) const { return memcmp(this, &o, sizeof(Shot)) == 0; }
};
enum { SHOT_NONE = 0, SHOT_KERNEL, SHOT_GENERIC, SHOT_REC };

template <class T> inline unsigned long long widen(T v) {
  static_assert(sizeof(T) <= 8, "an argument is a pointer, an int or a bool");
  unsigned long long w = 0;
  memcpy(&w, &v, sizeof(T));
  return w;
}
template <class... A> inline Shot shot(int what, const void* k, unsigned grid, unsigned block, A... args) {
  Shot s;
  memset(&s, 0, sizeof(s));
  s.k = k; s.what = what; s.grid = grid; s.block = block; s.nargs = (int)sizeof...(A);
  static_assert(sizeof...(A) <= 20, "arguments of a shot");
  const unsigned long long w[] = {widen(args)...};
  memcpy(s.a, w, sizeof(w));
  return s;
}

// per translation unit (the two sides of the check never share one)
static Shot g_shot;
static int g_shots;
static std::set<const void*> g_kernels;
static int g_capturing;
static inline void take(const Shot& s) {
  g_shot = s;
  ++g_shots;
  if (s.k) g_kernels.insert(s.k);
}
static unsigned int g_fake_queue[128 * 33 * 64];   // stands in for xw_disc_queue, slot by slot (its addresses only: never read or written)

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(K, G, B, SH, ST, ...) take(shot(SHOT_KERNEL, (const void*)(K), dim3(G).x, dim3(B).x, __VA_ARGS__))
#define xw_launch_status() 0
#define hipGetSymbolAddress(p, sym) (*(p) = (void*)g_fake_queue, hipSuccess)
#define hipStreamIsCapturing(s, p) (*(p) = g_capturing ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone, hipSuccess)

struct Tally {
  long cases, bad, kernel, generic, rec, error;
};
static inline void tally(Tally& t, const char* what, int rc, int rc_want, const Shot& want, const char* detail) {
  ++t.cases;
  t.kernel += g_shots == 1 && g_shot.what == SHOT_KERNEL; t.generic += g_shots == 1 && g_shot.what == SHOT_GENERIC;
  t.rec += g_shots == 1 && g_shot.what == SHOT_REC; t.error += rc != 0;
  const bool ok = rc == rc_want && g_shots == (want.what == SHOT_NONE ? 0 : 1) && (want.what == SHOT_NONE || g_shot == want);
  if (!ok && ++t.bad <= 10)
    printf("DISAGREE %s %s: rc %d (want %d), %d calls, kind %d k=%p grid=%u block=%u | want kind %d k=%p grid=%u block=%u\n", what, detail,
           rc, rc_want, g_shots, g_shot.what, g_shot.k, g_shot.grid, g_shot.block, want.what, want.k, want.grid, want.block);
}
