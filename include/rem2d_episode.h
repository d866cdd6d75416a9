#ifndef REM2D_EPISODE_H
#define REM2D_EPISODE_H

/* Episode boundaries for librem2d.so: a creature starts again the moment its episode ends, and the ended episode's result is
 * written down, on the device, for a WHOLE population (all lane buckets, all step groups) by one launch between two steps.
 * A header of its own, like include/rem2d_control.h and include/rem2d_policy.h: nothing here changes what a step computes,
 * REM2D_ABI_VERSION does not move, and the CPU twin (oracle/rem2d_cpu.c), which restates include/rem2d.h entry for entry, has
 * no counterpart of this call.
 *
 * The reference can only begin an episode for one individual at a time, by building its b2World again (Modular2D.reset,
 * Modular2DEnv.py:565-598); rem2d_world_reset does that for every creature of a world at once.  This call does it for SOME
 * creatures of many worlds, chosen by a mask, by the state the last step left, or both.  Creatures are independent b2Worlds, a
 * reset writes every field of a creature and nothing else, and every step writes the scratch it reads: a creature reset in
 * place continues bit for bit like the same creature in a freshly reset world, whatever its wavefront neighbours do.
 *
 * Joint targets (rem2d_worlds_control, rem2d_worlds_act) live in the controller words of the arena, which a reset takes from
 * the morphology again: a creature that was reset follows its own oscillators until the next control call. */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_EPISODE_ABI_VERSION 1

/* `when` conditions: a bit set of states in which a creature's episode counts as ended */
#define REM2D_WHEN_DONE   1  /* REM2D_F_DONE != 0 (the step just taken ended at the wall of death / behind x = 0) */
#define REM2D_WHEN_FROZEN 2  /* REM2D_F_FROZEN != 0 (evaluate()'s loop has ended: REM2D_main.py:362-377)          */
#define REM2D_WHEN_STEPS  4  /* max_steps > 0 && REM2D_F_STEPS >= max_steps (gym's TimeLimit)                    */

typedef struct {             /* caller-owned DEVICE arrays in population order, n_rows each; any may be NULL */
    float   *reward;         /* every creature: REM2D_F_REWARD as the last step left it (read before any reset) */
    uint8_t *done;           /* every creature: REM2D_F_DONE != 0, likewise                                     */
    uint8_t *ended;          /* every creature: 1 if this call reset it, else 0                                 */
    double  *fitness;        /* reset creatures only: REM2D_F_FITNESS of the episode that ended                 */
    int32_t *steps;          /* reset creatures only: REM2D_F_STEPS of it                                       */
    int32_t *episodes;       /* reset creatures only: += 1                                                      */
} rem2d_episode_out;

/* REM2D_EPISODE_ABI_VERSION of the library */
int rem2d_episode_abi_version(void);

/* Resets the SELECTED creatures of `worlds` (any number: one launch per 16 worlds) from morphs[i], the morphology of world i as
 * rem2d_world_reset took it (device pointers, [n_envs * lanes] each; the array of structs itself is host memory).
 *
 * Creature e of a world has population row r = index[e], `index` being the population index rem2d_world_set_outputs installed, or
 * r = e without one (as rem2d_worlds_observe finds it).  It is selected iff
 *     (mask_dev == NULL || mask_dev[r] != 0)  and  (when == 0 || one of the conditions named in `when` holds),
 * evaluated on the words the last step left.  mask_dev == NULL with when == 0 would select everyone: that is
 * rem2d_world_reset's job and is refused.  A creature whose row lies outside [0, n_rows) is never selected, and nothing is
 * written for it.
 *
 * A selected creature receives exactly what rem2d_world_reset writes for it: all its lanes, all its pair slots and all its
 * per-creature words (wall of death 0, fitness 0, step count 0, error bits 0, the controller words of the morphology, ...).
 * Unselected creatures, padding creatures, the alignment gaps of the arena and the arrays of rem2d_world_set_outputs are not
 * written.  Everything rem2d_world_reset keeps is kept: terrain, launch options, tile table, creature order, captured graphs,
 * timing state, hand-over counters.  `out` (or NULL) receives the harvest, read before anything is reset.
 *
 * Asynchronous on `stream`, on the device of the worlds; nothing is allocated.  Everything is checked before anything is
 * dereferenced or launched.  REM2D_E_INVALID: NULL worlds or morphs, n_worlds <= 0, unknown bits in `when`, REM2D_WHEN_STEPS
 * with max_steps <= 0, no mask and when == 0, n_rows < 0, a NULL world, a NULL array inside a morphology, a world of more
 * than 64 lanes per creature, worlds of several devices.  REM2D_E_STATE: a world before rem2d_world_reset (or adopt). */
int rem2d_worlds_reset_where(rem2d_world *const *worlds, const rem2d_morph *morphs /* [n_worlds], device pointers */,
                             int32_t n_worlds, const uint8_t *mask_dev /* [n_rows] or NULL */, uint32_t when,
                             int32_t max_steps, const rem2d_episode_out *out /* or NULL */, int64_t n_rows, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_EPISODE_H */
