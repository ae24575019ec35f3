/* xnwan_switches.h -- extension of the C ABI of libxnwan.so (include/xnwan.h, which stays as it is): the library's own switches,
 * the choices its entry points make besides what their arguments say.  The library reads no environment variable; a caller that
 * wants something else than the defaults says so here (the Python host: EngineOptions, kernels.apply_switches).
 *   disc_dynamic   : 1  xw_disc_fwd / xw_disc_fwd_xproj deal the tiles of a launch with more than one round per wave from ticket
 *                       queues; 0: a static split
 *   disc_vin_lds   : 1  ... keep the input layer's fragments in LDS at the widths 50 and 64 (no x-projection table given);
 *                       0: load them from global memory
 *   disc_rec_tsum  : 1  xw_disc_bwd from the record sums the input layer's gradient once per 64-path group on vertical paths;
 *                       0: per tile.  This changes the order of that sum, and so the last bits of the gradient
 *   duo_spread     : 1  the duo sweep of xw_ode_bwd_multi launches a spacer round of empty blocks between its rounds of tiles
 *   reduce_blocks  : block cap of the deterministic grid sums (xw_weak_partials, xw_bdry_partials); 0: by size -- 128, or 256
 *                       above 2^18 points
 *   reduce_threads : their block size, 256, 512 or 1024
 * Defaults: {1, 1, 1, 1, 0, 1024}.
 * The value is process-wide and host-only.  Every launch call reads it when it is called, unsynchronised: set it between launch
 * calls, not concurrently with them.  A launch that was recorded into a graph keeps what was chosen at capture.
 * xw_switches_set returns XW_E_ARG and changes nothing for a null pointer, a flag other than 0 or 1, reduce_blocks outside
 * 0..1024 or reduce_threads not one of 256, 512, 1024; xw_switches_get returns XW_E_ARG for a null pointer. */
#ifndef XNWAN_SWITCHES_H
#define XNWAN_SWITCHES_H
#include "xnwan.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct { int disc_dynamic, disc_vin_lds, disc_rec_tsum, duo_spread, reduce_blocks, reduce_threads; } XwSwitches;
int xw_switches_set(const XwSwitches* s);
int xw_switches_get(XwSwitches* s);

#ifdef __cplusplus
}
#endif
#endif
