#ifndef REM2D_STREAM_H
#define REM2D_STREAM_H

/* Streaming evaluation for librem2d.so: a slot whose creature has finished takes the NEXT creature of a pending queue, on the
 * device, for a whole population (all lane buckets, all step groups) by one launch between two steps.  A population of any size
 * runs through a fixed window of slots; nothing waits in an arena of its own for its turn or for the others to finish.
 * A header of its own, like include/rem2d_episode.h: nothing here changes what a step computes, REM2D_ABI_VERSION does not move,
 * and the CPU twin (oracle/rem2d_cpu.c), which restates include/rem2d.h entry for entry, has no counterpart of this call.
 *
 * Why a slot can change its creature between two steps.  (1) The state depends on the morphology only through the reset:
 * rem2d_world_reset writes every field of a creature from its own lanes' 20 morphology words and nothing else, and every step
 * writes the scratch it reads.  (2) The tile table of a FLEXIBLE tile shape (1, 2, 3; rem2d_world_set_tile_shape) does not depend
 * on the morphology: rem2d_plan_tiles_shape closes a tile when the creature cap is reached or when more than sets x 64 joints are
 * in it; such a tile holds at most passes x 64 <= sets x 64 lanes and a creature has fewer joints than lanes, so the table is a
 * function of (n_envs, lanes, n_padded, max_creatures) alone.  The static shapes 0 and 4 plan from the joints per schedule phase:
 * worlds on them are refused here.  A new occupant must have the slot's lane count.
 *
 * Conditions: the REM2D_WHEN_* bits of include/rem2d_episode.h, evaluated on the same words. */

#include "rem2d_episode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_STREAM_ABI_VERSION 1

typedef struct {            /* pending creatures of ONE lane count, caller-owned DEVICE memory */
    rem2d_morph M;          /* [count * lanes] each, lane fastest, exactly as rem2d_world_reset takes them */
    const int32_t *id;      /* [count]: result row of pending creature q */
    int32_t count, lanes;
    int32_t *cursor;        /* device word: pending creatures handed out so far; the call advances it */
} rem2d_feed;

typedef struct {            /* DEVICE arrays indexed by id, n_ids each; any may be NULL */
    double *fitness; int32_t *steps; int32_t *err; uint8_t *finished;
} rem2d_stream_out;

/* REM2D_STREAM_ABI_VERSION of the library */
int rem2d_stream_abi_version(void);

/* Harvests the creatures of `worlds` (any number: one launch per 8 worlds) whose episode has ended, and gives their slots to the
 * next pending creatures of feeds[i], the feed of world i.  morphs[i] is the morphology of world i as rem2d_world_reset took it
 * (device pointers, [n_envs * lanes] each; the arrays of structs themselves are host memory): the call WRITES the new occupant's
 * words into it, so that a later rem2d_worlds_reset_where restarts the creature that is in the slot now.
 *
 * Creature e of a world has population row r = index[e] (the index of rem2d_world_set_outputs, or r = e without one), as
 * rem2d_worlds_reset_where finds it; rows outside [0, n_rows) are left alone.  occ = occupant_dev[r] is the id of the creature
 * in that slot, -1 = the slot is empty.
 *   1. ended = occ >= 0 && one of the conditions named in `when` holds (when == 0 is refused).
 *   2. ended and 0 <= occ < n_ids: out.fitness[occ] = REM2D_F_FITNESS, out.steps[occ] = REM2D_F_STEPS, out.err[occ] =
 *      REM2D_F_ERR, out.finished[occ] = 1 -- read before any store of 3.
 *   3. ended: q = the feed's cursor, post-incremented (one atomic add per wavefront).  q < count: the 20 words of every lane of
 *      pending creature q are copied into morphs[i] at the slot's lanes, every lane is reset from the words it copied (exactly
 *      what rem2d_world_reset writes for it), and occupant_dev[r] = id[q].  Otherwise the slot is retired: occupant_dev[r] = -1
 *      and REM2D_F_FROZEN = 1 (under REM2D_FLAG_SKIP_FROZEN a wavefront of retired slots stops being stepped), nothing else.
 *   4. Creatures that have not ended, empty slots, padding creatures, the alignment gaps of the arena and the arrays of
 *      rem2d_world_set_outputs are not written.
 * Worlds of one lane count may share a feed AND its cursor.  Which pending creature lands in which slot is unspecified:
 * occupant_dev is the record.  Every value indexed by id is deterministic, because creatures are independent.  The cursor may run
 * past `count`: readers clamp it.  A feed with count == 0 may carry NULL arrays: the call then only harvests and retires.
 *
 * Everything rem2d_world_reset keeps is kept: terrain, launch options, tile table, creature order, captured graphs, timing state,
 * hand-over counters.  `out` may be NULL (nothing is harvested).  Asynchronous on `stream`, on the device of the worlds; nothing is
 * allocated.  Everything is checked before anything is dereferenced or launched.  REM2D_E_INVALID: NULL worlds, morphs, feeds or occupant_dev, n_worlds <= 0, when == 0 or
 * unknown bits in it, REM2D_WHEN_STEPS with max_steps <= 0, n_rows < 0 or n_ids < 0, a NULL world, a NULL array inside a
 * morphology, a feed with count < 0, without a cursor, with count > 0 and a NULL array or id, or with lanes other than its
 * world's, a world of more than 64 lanes per creature, worlds of several devices.  REM2D_E_STATE: a world before
 * rem2d_world_reset (or adopt); a world on a static tile shape (0 or 4), whose tile table is planned from the joints. */
int rem2d_worlds_refill(rem2d_world *const *worlds, const rem2d_morph *morphs, int32_t n_worlds,
                        const rem2d_feed *feeds /* [n_worlds]; worlds of one lane count may share a feed AND its cursor */,
                        int32_t *occupant_dev /* [n_rows], population-row order: id in that slot, -1 = empty */,
                        uint32_t when, int32_t max_steps, const rem2d_stream_out *out, int64_t n_ids,
                        int64_t n_rows, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_STREAM_H */
