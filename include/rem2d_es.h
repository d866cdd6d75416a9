#ifndef REM2D_ES_H
#define REM2D_ES_H

/* An evolution strategy for device policies for librem2d.so: antithetic sampling around one mean controller per morphology, rank
 * shaping of the episode fitness and the rank-weighted update of the mean, on the device, for a WHOLE population.  A header of its
 * own, like rem2d_evolve.h: nothing here changes what a step, an observation row, a forward pass or rem2d_policy_evolve holds.
 *
 * Layout.  G = M S child weight sets w1[D][H], b1[H], w2[H][MB], b2[MB] (binary32, as rem2d_policy lays them out) form M blocks of
 * S = group_size consecutive sets (creatures that share a morphology are the caller's blocks); S is even and at least 2.  The mean
 * has M sets of the same per-set shapes, one per block.  Child c = b S + j belongs to pair q = j >> 1 of block b; the pair's anchor
 * is a = b S + 2 q, its even child.  All buffers are device memory the caller owns.
 *
 * Draw.  Philox4x32-10 exactly as rem2d_evolve.h states it (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 * 0xBB67AE85, ten rounds).  key = (seed & 0xffffffff, seed >> 32); counter = (i, a, generation, 4 + k), k = 1, 2, 3, 4 for w1, b1,
 * w2, b2 -- the domains 5 .. 8, disjoint from rem2d_evolve's 0 .. 4 -- a the pair's anchor and i the element's index inside that
 * array of ONE set.  With the output words x0 .. x3:
 *   s = the sum of the six 16-bit halves of x1, x2, x3, minus 196605   (an int32 in -196605 .. 196605; x0 is unused)
 *   z = (float)s * C,  C = the binary32 constant 0x37B504F3 (fl32(sqrt 2) * 2^-16): unit variance, support +-4.24.
 * A draw is a function of (seed, generation, a, k, i) alone: no state, no order, and nobody has to store it.
 *
 * Sample (rem2d_es_sample) writes every child word from the mean's word m of its block:
 *   even j:  m + (sigma * z)            odd j:  m + (-(sigma * z))
 * Each product and each sum is one correctly rounded binary32 operation, nothing is fused, in any build of the library.  Where
 * the result is a NaN (a NaN mean word, inf * 0, inf - inf) its sign and payload are undefined, as IEEE 754 leaves them.
 *
 * Shape (rem2d_es_shape) turns fitness[G] (binary64) into util[G] (int32) within each block, on rem2d_evolve's order on fitness:
 * every NaN equals every other NaN and is below everything else; -0 == +0; otherwise the usual order.  For child c,
 *   util[c] = 2 L + E - (S - 1),   L = the number of OTHER sets of c's block strictly below c,
 *                                  E = the number of OTHER sets of the block neither above nor below c:
 * centred ranks with ties averaged, times 2 (S - 1), as integers in -(S - 1) .. S - 1.  A block's util sums to 0; a block of equal
 * or all-NaN fitness gives zeros.  Example, S = 6: [NaN, 1, 1, -0, +0, inf] gives [-5, 2, 2, -2, -2, 5].
 *
 * Update (rem2d_es_update) reads util, which the caller may have filled, never a child word and never a stored draw:
 *   d_q = util[a] - util[a + 1]                       an int32 (modulo 2^32; util of rem2d_es_shape: |d_q| <= 2 (S - 1), exact)
 *   g_i = the sum over the block's pairs q of d_q * s_{q,i}   an EXACT int64: with util of rem2d_es_shape |g_i| <= S^2 * 2^18
 *                                                      (2^50 at S = 65536).  Integer sums are associative: the result does not
 *                                                      depend on how the pairs are dealt over lanes, wavefronts or launches.
 *                                                      (A caller's util that takes the sum past 2^63 wraps modulo 2^64.)
 *   new mean word = m + (step * ((float)(double)g_i * C))
 * int64 -> binary64 is exact below 2^53 (round to nearest even above), binary64 -> binary32 one rounding, then two separately
 * rounded products and one rounded sum.  step is a binary32 the caller computes: for the update
 * mean += lr / (S sigma) * sum_c rank_c z_c of centred ranks in [-1/2, 1/2] it is fl32(lr / (2 (S - 1) S sigma)).  The new mean is
 * written to buffers of its own, which may not overlap the old mean's.
 *
 * With few blocks of many sets the pairs of a block are split into chunks of pair_chunk pairs over wavefronts, whose int64 partial
 * sums go through `scratch` and are summed by a finishing launch.  pair_chunk = 0 leaves the choice to the library; any other
 * value is the number of pairs per wavefront (a value of S / 2 or more: no split).  No result depends on it.
 * rem2d_es_scratch_bytes states what `scratch` must hold for a descriptor (0: no split, scratch may be NULL).
 *
 * A host model reproduces every bit (tests/es_model.py).  The library allocates nothing; all calls are asynchronous on `stream`,
 * on the device that is current. */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_ES_ABI_VERSION 1

/* Caller-owned device pointers and the shapes they have. */
typedef struct rem2d_es {
    int32_t d;              /* D: input rows of w1, 8 + 6 max_bodies + R with R in 0 .. 64 (REM2D_SENSE_MAX_RAYS) */
    int32_t hidden;         /* H: 1 .. 128 (REM2D_POLICY_MAX_HIDDEN) */
    int32_t max_bodies;     /* MB: 1 .. 64 (REM2D_CONTROL_MAX_BODIES) */
    int32_t n_means;        /* M >= 1 blocks: sets of the mean */
    int32_t group_size;     /* S: even, >= 2; M S <= 2^31 - 1 child sets */
    int32_t pair_chunk;     /* >= 0: pairs per wavefront of the update, 0 = the library's choice */
    uint32_t generation;    /* counter word 2 */
    int32_t reserved;       /* 0 */
    uint64_t seed;          /* the Philox key */
    float sigma;            /* sampling step; read by sample */
    float step;             /* update step; read by update and step */
    const double *fitness;  /* [M S]; read by shape and step */
    int32_t *util;          /* [M S]; written by shape and step, read by update */
    const float *w1;        /* [M][D][H]   the mean; read by sample, update and step */
    const float *b1;        /* [M][H] */
    const float *w2;        /* [M][H][MB] */
    const float *b2;        /* [M][MB] */
    float *child_w1;        /* [M S][D][H]   the children, written by sample; none may overlap a buffer of the mean */
    float *child_b1;        /* [M S][H] */
    float *child_w2;        /* [M S][H][MB] */
    float *child_b2;        /* [M S][MB] */
    float *new_w1;          /* [M][D][H]   the new mean, written by update and step; none may overlap a buffer of the mean */
    float *new_b1;          /* [M][H] */
    float *new_w2;          /* [M][H][MB] */
    float *new_b2;          /* [M][MB] */
    void *scratch;          /* scratch_bytes bytes, 8-byte aligned, for update and step; NULL where rem2d_es_scratch_bytes is 0 */
    uint64_t scratch_bytes; /* what `scratch` holds: at least rem2d_es_scratch_bytes(e) */
} rem2d_es;

/* REM2D_ES_ABI_VERSION of the library */
int rem2d_es_abi_version(void);

/* Bytes of scratch that rem2d_es_update and rem2d_es_step need for e (its shapes, n_means, group_size and pair_chunk; no pointer
 * is looked at), 0 where the pairs are not split; REM2D_E_INVALID (negative) for a NULL e, a dimension out of range (the limits of
 * rem2d_policy), n_means < 1, a group_size that is odd or below 2, n_means * group_size above 2^31 - 1, a negative pair_chunk, a
 * non-zero reserved. */
int64_t rem2d_es_scratch_bytes(const rem2d_es *e);

/* The children of one generation: one kernel that reads every word of the mean and writes every child word once.
 * REM2D_E_INVALID for what rem2d_es_scratch_bytes refuses, a NULL mean or child pointer, a child buffer that overlaps a buffer of
 * the mean.  fitness, util, the new mean and scratch are not looked at. */
int rem2d_es_sample(const rem2d_es *e, void *stream);

/* util[c] for every child, one kernel.  REM2D_E_INVALID for what rem2d_es_scratch_bytes refuses, a NULL fitness or util.  The
 * weight pointers and scratch are not looked at. */
int rem2d_es_shape(const rem2d_es *e, void *stream);

/* The new mean from the mean and whatever e->util holds: one kernel, or two where the pairs are split.  REM2D_E_INVALID for what
 * rem2d_es_scratch_bytes refuses, a NULL util, mean or new-mean pointer, a new-mean buffer that overlaps a buffer of the mean, a
 * scratch that is NULL, not 8-byte aligned or smaller than rem2d_es_scratch_bytes(e) where that is not 0.  fitness and the
 * children are not looked at. */
int rem2d_es_update(const rem2d_es *e, void *stream);

/* rem2d_es_shape, then rem2d_es_update: two or three launches queued by one call.  Everything is checked before the first. */
int rem2d_es_step(const rem2d_es *e, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_ES_H */
