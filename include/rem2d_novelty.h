#ifndef REM2D_NOVELTY_H
#define REM2D_NOVELTY_H

/* Behavioural novelty for librem2d.so: a behaviour descriptor recorded on the device while an episode runs, a k-nearest-neighbour
 * novelty score of every descriptor against its block's peers and an archive, and the archive's upkeep.  A header of its own, like
 * the evolve and the evolution-strategy headers: nothing here changes what a step, an observation row, a forward pass or a search
 * operator holds.  The CPU twin has no counterpart of anything in this header.
 *
 * ---- 1. The descriptor (rem2d_worlds_describe) ----
 * A row of K = n_samples slots of two binary32 words, [out_rows][2 K]: words 2 k and 2 k + 1 of a creature's row are slot k.  Rows
 * are found as rem2d_worlds_observe finds them (the rem2d_world_set_outputs index, or the identity); rows outside [0, out_rows) are
 * skipped.  The call keeps no state.  Let s be the creature's REM2D_F_STEPS word.
 *   A creature whose episode is running writes (px_root, py_root) -- the binary32 words rem2d_worlds_observe copies to head words 0
 *   and 1 -- to EVERY slot k < K with (k + 1) * period >= s, and touches no lower slot.
 *   A creature whose episode is over writes nothing.
 * "Over" is REM2D_F_FROZEN != 0, and nothing else.  The step's bookkeeping sets DONE only together with a reward of -100, which
 * freezes the creature in the same step, and EVERDONE only with DONE: both imply FROZEN from that step on, so neither adds a case.
 * (A creature that is over but shares a wavefront with running ones is still stepped -- REM2D_FLAG_SKIP_FROZEN skips only
 * wavefronts in which everyone is frozen -- so its later positions depend on its neighbours; the descriptor is a function of the
 * creature alone, which is why the skip is part of the contract.)
 * So slot k ends up holding the root position at the last call made with s <= (k + 1) * period while the episode ran: a call right
 * after a reset (s = 0) fills the whole row with the start position, an episode that ends early carries its last recorded position
 * forward, and with one call per `period` steps slot k is the position at step (k + 1) * period.
 *
 * ---- 2. The score (rem2d_novelty_score) ----
 * desc[G][B] (binary32), G = n_rows rows of B = width words, in M = G / S blocks of S = group_size consecutive rows.  The archive
 * holds cap = capacity entries of B words per block, archive[M][cap][B]; total[b] counts the entries ever added to block b and the
 * entries e < min(total[b], cap) are live.  For row c of block b, with x = desc[c]:
 *   d2(x, y):  d2 = 0.0f;  for i = 0 .. B - 1 ascending:  t = x_i - y_i;  d2 = d2 + (t * t)
 *              every difference, product and sum one correctly rounded binary32 operation, nothing fused, in any build of the
 *              library.  d2(x, y) and d2(y, x) are the same bits.
 *   candidates: the OTHER rows of block b (c excluded by its index, not by its value) and the live archive entries of block b.  A
 *              candidate whose d2 is not finite (a NaN or infinite word, an overflow) is ignored.
 *   k' = min(k, the number of finite candidates);  v_0 <= ... <= v_{k'-1} the k' smallest d2
 *   novelty[c] = ( sum over j = 0 .. k'-1 ascending, in binary64, of (double)sqrtf(v_j) ) / (double)k'
 *              sqrtf the correctly rounded binary32 root.  k' = 0 gives 0.0.  If a word of x itself is not finite the result is a
 *              NaN whose sign and payload are undefined.
 * The result depends on the multiset of the k' smallest values alone: no tie-break exists or is needed, and nothing depends on the
 * launch shape.
 * Example (B = 1, S = 4, k = 2, one live archive entry 10):  desc = [0, 3, 4, 8]
 *   row 0: d2 = {9, 16, 64, 100} -> (3 + 4) / 2 = 3.5      row 1: {9, 1, 25, 49} -> (1 + 3) / 2 = 2
 *   row 2: {16, 1, 16, 36} -> (1 + 4) / 2 = 2.5            row 3: {64, 25, 16, 4} -> (2 + 4) / 2 = 3
 *
 * ---- 3. The archive (rem2d_novelty_add) ----
 * Row c is ADDED iff all its words are finite, and add_mask == NULL or add_mask[c] != 0, and (uint64)x0 < add_threshold, x0 the
 * first output word of Philox4x32-10 exactly as the evolve header states it (multipliers 0xD2511F53 / 0xCD9E8D57, key increments
 * 0x9E3779B9 / 0xBB67AE85, ten rounds) with key = (seed & 0xffffffff, seed >> 32) and counter = (0, c, generation, 9): domain 9,
 * disjoint from the domains 0 .. 8 of the two search headers.  add_threshold = floor(rate * 2^32): 0 adds nothing, 2^32 adds every
 * admissible row.
 * The j-th added row of block b, in ascending row order, goes to entry (total[b] + j) mod cap; where a call adds n > cap rows to a
 * block only the last cap of them (j >= n - cap) are written.  Then total[b] += n.  With cap = 0 nothing is written and total
 * still counts.  total[b] must not be negative.
 * Examples (cap = 3, B = 1):  total = 2, rows 5, 6 added: entry 2 = 5, entry 0 = 6, total = 4 (the ring wraps).
 *                             total = 1, rows 1, 2, 3, 4, 5 added: 1 and 2 are not written; entry 0 = 3, 1 = 4, 2 = 5; total = 6.
 *
 * rem2d_novelty_step is the score, then the add, queued by one call: the score sees the archive as it was before the add.
 *
 * A host model reproduces every bit (tests/novelty_model.py).  The library allocates nothing; all calls are asynchronous on
 * `stream`, on the device that is current (rem2d_worlds_describe: the worlds' device). */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_NOVELTY_ABI_VERSION 1
#define REM2D_NOVELTY_MAX_WIDTH 32   /* B */
#define REM2D_NOVELTY_MAX_K 32       /* k */
#define REM2D_NOVELTY_MAX_SAMPLES 16 /* K of rem2d_worlds_describe: a row of 2 K <= REM2D_NOVELTY_MAX_WIDTH words */

/* Caller-owned device pointers and the shapes they have. */
typedef struct rem2d_novelty {
    int32_t width;          /* B: 1 .. 32 */
    int32_t n_rows;         /* G >= 1 */
    int32_t group_size;     /* S >= 1, dividing G */
    int32_t k;              /* neighbours: 1 .. 32 */
    int32_t capacity;       /* cap >= 0 archive entries per block */
    uint32_t generation;    /* counter word 2 of the add */
    uint64_t seed;          /* the Philox key of the add */
    uint64_t add_threshold; /* 0 .. 2^32 */
    const float *desc;      /* [G][B]; read by all three */
    float *archive;         /* [M][cap][B]; read by score, written by add; NULL where cap is 0; may not overlap desc */
    int64_t *total;         /* [M]; read by score, read and written by add */
    double *novelty;        /* [G]; written by score and step; not looked at by add; may not overlap desc */
    const uint8_t *add_mask; /* [G] or NULL; read by add */
    int32_t reserved;       /* 0 */
} rem2d_novelty;

/* REM2D_NOVELTY_ABI_VERSION of the library */
int rem2d_novelty_abi_version(void);

/* The descriptor rows of every creature of the worlds: one launch per 16 worlds.  REM2D_E_INVALID for period < 1, n_samples outside
 * 1 .. 16 and what rem2d_worlds_observe refuses (no worlds, a NULL world or buffer, negative out_rows, more than 64 lanes per
 * creature, worlds on several devices); REM2D_E_STATE for a world that was never reset.  Everything is checked before anything is
 * dereferenced or launched. */
int rem2d_worlds_describe(rem2d_world *const *worlds, int32_t n_worlds, int32_t period, int32_t n_samples, float *out_dev,
                          int64_t out_rows, void *stream);

/* novelty[c] for every row: one kernel.  REM2D_E_INVALID for a NULL descriptor, a dimension out of range, a group_size that does
 * not divide n_rows, an add_threshold above 2^32, a non-zero reserved, a NULL desc, total or novelty, a NULL archive where capacity
 * is not 0, an archive or novelty that overlaps desc. */
int rem2d_novelty_score(const rem2d_novelty *n, void *stream);

/* The archive's upkeep: one kernel, a workgroup per block.  REM2D_E_INVALID as rem2d_novelty_score, except that novelty is not
 * looked at. */
int rem2d_novelty_add(const rem2d_novelty *n, void *stream);

/* rem2d_novelty_score, then rem2d_novelty_add: two launches queued by one call.  Everything is checked before the first. */
int rem2d_novelty_step(const rem2d_novelty *n, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_NOVELTY_H */
