#ifndef REM2D_GATHER_H
#define REM2D_GATHER_H

/* Device-side read-back helpers of librem2d.so for a front-end that splits one population over several worlds
 * (gym_rem2d_amd.env.BatchedModular2D).  Kept apart from include/rem2d.h: that header is the world ABI the CPU twin
 * (oracle/rem2d_cpu.c) restates entry for entry, and a population-order copy between device buffers has nothing to
 * restate on host pointers. */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Population-order copy of a per-creature field (REM2D_F_WOD .. REM2D_F_TOIEVENTS): out_dev[index[e]] = field[e] for the
 * world's n_envs creatures, where `index` is the int32 device array rem2d_world_set_outputs installed (REM2D_E_STATE without
 * one).  out_dev holds out_count elements of the field's own type (REM2D_DT_*: 4 or 8 bytes, copied bit for bit); an index
 * outside [0, out_count) is skipped.  Device pointers; asynchronous on `stream`.  One small kernel of this library: nothing is
 * loaded or allocated on a first call. */
int rem2d_world_gather(const rem2d_world *w, int32_t field, void *out_dev, int64_t out_count, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_GATHER_H */
