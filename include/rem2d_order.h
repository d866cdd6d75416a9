#ifndef REM2D_ORDER_H
#define REM2D_ORDER_H

/* The creature order of a world, read back and made on demand, for librem2d.so.  A header of its own, like include/rem2d_episode.h and
 * include/rem2d_stream.h: nothing here changes what a step computes or launches, REM2D_ABI_VERSION does not move, and the CPU twin
 * (oracle/rem2d_cpu.c), which restates include/rem2d.h entry for entry, has no counterpart of these calls (it has no launch shapes).
 *
 * The step kernels of a world whose order is in use (rem2d_world_set_order installed one, or REM2D_OPT_REBALANCE > 0) find the creature
 * of slot e in an int array of the library's own, outside the state arena: two halves of n_padded = rem2d_padded_envs() ints each,
 * half 0 what the kernels read, half 1 its copy (REM2D_FLAG_RETILE worlds swap them; all others keep them equal).  Both halves are a
 * permutation of 0 .. n_envs - 1 followed by the padding slots n_envs .. n_padded - 1, which hold themselves.  A duplicate would make two
 * slots step one creature and leave another unstepped, with nothing to show for it: these two calls are what lets a test look.
 *
 * The order REM2D_OPT_REBALANCE re-makes every N env-steps is a STABLE counting sort of 0 .. n_envs - 1 by cost class of the creature's
 * last step (REM2D_F_POSITERS p, against the position iterations `pos_iters` of the step call):
 *     class 0: p >= pos_iters        class 1: 3 <= p < pos_iters        class 2: the rest
 * -- one workgroup per world, of 64 threads, doubled while fewer than 1 024 and threads * 256 < n_envs. */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_ORDER_ABI_VERSION 1

/* REM2D_ORDER_ABI_VERSION of the library */
int rem2d_order_abi_version(void);

/* Copies both halves of the world's creature order, 2 * n_padded ints, to `out_dev` (device memory of the world's device),
 * device-to-device and asynchronously on `stream` -- behind whatever that stream has queued for the world.  It reads the array as it
 * is, whether or not the kernels go through it at the moment.  REM2D_E_INVALID: NULL world or NULL `out_dev`. */
int rem2d_world_read_order(const rem2d_world *w, int32_t *out_dev, void *stream);

/* Makes the world's order from the state in place, now: ONE launch of the re-ordering kernel on `stream`, by the launch code the step
 * calls use every N steps, thread-count rule included.  Nothing else: the cadence of REM2D_OPT_REBALANCE (the steps queued so far, the
 * steps at the last re-ordering), whether the kernels go through the order, every option and every captured graph stay as they are --
 * a world that does not use its order is stepped exactly as before.  REM2D_E_INVALID: NULL world, a REM2D_FLAG_RETILE world (it deals
 * its creatures itself, as for rem2d_world_set_order), pos_iters < 1. */
int rem2d_world_make_order(rem2d_world *w, int32_t pos_iters, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_ORDER_H */
