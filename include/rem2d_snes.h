#ifndef REM2D_SNES_H
#define REM2D_SNES_H

/* An adaptive evolution strategy for device policies for librem2d.so: the sampling of the evolution strategy (the ES header,
 * beside this one) with a step size PER PARAMETER -- a separable natural evolution strategy: every word of the mean has a sigma
 * word of its own, adapted from the same utilities -- and, on request, Adam on the mean.  A header of its own, like the ES
 * header: nothing here changes what the ES calls compute.
 *
 * Layout and draw: exactly those of the ES header.  G = M S child weight sets in M blocks of S = group_size consecutive sets,
 * S even and at least 2; child c = b S + j belongs to pair q = j >> 1 of block b, whose anchor is a = b S + 2 q.  Philox4x32-10
 * (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds), key = (seed & 0xffffffff, seed >> 32),
 * counter =
 * (i, a, generation, 4 + k), k = 1, 2, 3, 4 for w1, b1, w2, b2 (the domains 5 .. 8), i the element's index inside that array of ONE
 * set.  s = the sum of the six 16-bit halves of x1, x2, x3, minus 196605 (an int32 in -196605 .. 196605), z = (float)s * C, C the
 * binary32 constant 0x37B504F3.  The draws are deliberately the ES's: a run uses one strategy or the other.
 *
 * Group size: S <= 8192 (REM2D_SNES_MAX_GROUP), see h_i below.
 *
 * State, per block, binary32, each of the mean's per-set shapes ([M][D][H], [M][H], [M][H][MB], [M][MB]): sigma; m1 and m2 (Adam's
 * moments) with REM2D_SNES_ADAM only.
 *
 * Sample (rem2d_snes_sample) writes every child word from the mean's word m and the sigma word sg of its block:
 *   even j:  m + (sg * z)            odd j:  m + (-(sg * z))
 * Each product and each sum is one correctly rounded binary32 operation, nothing is fused, in any build of the library.
 *
 * Update (rem2d_snes_update) reads util (int32 [M S], which the caller may have filled; the ES shape call makes the ranks),
 * the mean and the state, never a child word and never a stored draw.  Per pair
 *   d_q = util[a] - util[a + 1]          p_q = util[a] + util[a + 1]          (int32, modulo 2^32)
 * and per element i of a block, both sums wrapping modulo 2^64,
 *   g_i = sum over q of d_q * s_{q,i}                 |g_i| <= S^2 * 2^18 for util of the ES shape call (2^44 at S = 8192)
 *   h_i = sum over q of p_q * (s_{q,i}^2 - 2^31)      |p_q| <= 2 (S - 1), |s^2 - 2^31| < 2^35.1 (s^2 < 2^35.17), S / 2 pairs:
 *                                                     |h_i| <= S^2 * 2^35.1 for util of the ES shape call, below 2^62 at S = 8192
 *                                                     and past 2^63 above that size: hence the limit.
 * Both are exact int64 for the util of the ES shape call; integer sums are associative, so no result depends on how the pairs are
 * dealt over lanes, wavefronts or launches.  A pair is skipped only where d_q == 0 AND p_q == 0 (a level pair,
 * util[a] == util[a + 1] != 0, has d_q == 0 and still moves sigma).  E[s^2] is 2^31 - 1/2, not 2^31: the half, times the sum of a
 * block's p_q, cancels exactly wherever the block's util sums to 0, which holds for the util of the ES shape call.
 *
 * Conversions (int64 -> binary64 round to nearest even, binary64 -> binary32 one rounding, one product each):
 *   G  = (float)(double)g_i * C
 *   Hh = (float)(double)h_i * 2^-31
 * Sigma, with the caller's binary32 sstep, sigma_min, sigma_max and the old sigma word sg:
 *   x   = sstep * Hh;  a NaN x becomes 0, otherwise x is clamped to [-1, 1]
 *   f   = (2 + x) / (2 - x)            the (1,1) Pade form of exp(x): correctly rounded +, -, / alone (no exp, which no two
 *                                      libraries round alike); f lies in [1/3, 3] and is positive
 *   sg' = sg * f
 *   sg' = sg' < sigma_min ? sigma_min : (sg' > sigma_max ? sigma_max : sg')          (a NaN passes through)
 * Mean, with the caller's binary32 mstep, beta1, omb1, beta2, omb2, alpha, eps and the old words m, m1, m2:
 *   t   = (flags & REM2D_SNES_NATURAL) ? sg * G : G                                   (the OLD sigma)
 *   without REM2D_SNES_ADAM:  m' = m + (mstep * t)
 *   with REM2D_SNES_ADAM:     gh  = mstep * t
 *                             m1' = (beta1 * m1) + (omb1 * gh)
 *                             m2' = (beta2 * m2) + (omb2 * (gh * gh))
 *                             m'  = m + (alpha * (m1' / (sqrtf(m2') + eps)))
 * Every operation is rounded separately, in every build; sqrtf and / are correctly rounded.  Adam's bias correction is folded into
 * alpha by the caller: alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t) at update t = 1, 2, ...  For the update
 * mean += lr / (S sigma0) * sum_c rank_c z_c of centred ranks in [-1/2, 1/2], mstep is fl32(lr / (2 (S - 1) S sigma0)); for
 * log sigma += lr_sigma / (2 S) * sum_c rank_c (z_c^2 - 1), sstep is fl32(lr_sigma / (4 (S - 1) S)).
 *
 * Example: S = 2, util = [3, 1] (d = 2, p = 4), s = 1000 for some element: g = 2000, h = 4 (10^6 - 2^31) = -8585934592;
 * fl32(h) = -8585934848, Hh = -3.9981374740600586; with sstep = 0.125 x = -0.4997671842575073,
 * f = fl32(1.5002328157424927 / 2.499767303466797) = 0x3F19A35D (0.6001489758491516); sg = 0.1f gives sg' = 0x3D75D22F
 * (0.06001489982008934), and G = 2000 * C = 0x3D30C6D5 (0.04315837100148201).
 *
 * Outputs: the new mean and the new sigma go to buffers of their own, and with REM2D_SNES_ADAM so do the new m1 and m2.  No output
 * may overlap any input or any other output, so a call can be repeated on the same inputs.
 *
 * With few blocks of many sets the pairs of a block are split into chunks of pair_chunk pairs over wavefronts, exactly as
 * the ES header says (0: the library's choice, the same choice as the ES update's); the scratch then holds TWO int64 per
 * element per chunk, [block][chunk][2][E], and a finishing launch sums them and applies the result.
 *
 * A host model reproduces every bit (tests/snes_model.py).  The library allocates nothing; all calls are asynchronous on `stream`,
 * on the device that is current. */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_SNES_ABI_VERSION 1
#define REM2D_SNES_MAX_GROUP 8192

#define REM2D_SNES_ADAM 1u     /* Adam on the mean: m1, m2 and their outputs are read and written */
#define REM2D_SNES_NATURAL 2u  /* the mean's step is scaled by the element's (old) sigma */

/* Caller-owned device pointers and the shapes they have. */
typedef struct rem2d_snes {
    int32_t d;              /* D: input rows of w1, 8 + 6 max_bodies + R with R in 0 .. 64 */
    int32_t hidden;         /* H: 1 .. 128 */
    int32_t max_bodies;     /* MB: 1 .. 64 */
    int32_t n_means;        /* M >= 1 blocks */
    int32_t group_size;     /* S: even, 2 .. REM2D_SNES_MAX_GROUP; M S <= 2^31 - 1 */
    int32_t pair_chunk;     /* >= 0: pairs per wavefront of the update, 0 = the library's choice */
    uint32_t generation;    /* counter word 2 */
    uint32_t flags;         /* REM2D_SNES_ADAM | REM2D_SNES_NATURAL; no other bit */
    uint64_t seed;          /* the Philox key */
    float mstep;            /* the mean's step */
    float sstep;            /* sigma's step */
    float beta1;            /* Adam: read with REM2D_SNES_ADAM only, as are omb1 .. eps */
    float omb1;             /* 1 - beta1, as the caller rounds it */
    float beta2;
    float omb2;             /* 1 - beta2 */
    float alpha;            /* Adam's step with the bias correction folded in */
    float eps;
    float sigma_min;        /* finite, 0 < sigma_min <= sigma_max; read by update and step */
    float sigma_max;
    const double *fitness;  /* [M S]; read by step */
    int32_t *util;          /* [M S]; written by step, read by update */
    const float *w1;        /* [M][D][H]   the mean; read by sample, update and step */
    const float *b1;        /* [M][H] */
    const float *w2;        /* [M][H][MB] */
    const float *b2;        /* [M][MB] */
    const float *sigma_w1;  /* sigma, the mean's shapes; read by sample, update and step */
    const float *sigma_b1;
    const float *sigma_w2;
    const float *sigma_b2;
    const float *m1_w1;     /* Adam's first moment, the mean's shapes; read by update and step with REM2D_SNES_ADAM */
    const float *m1_b1;
    const float *m1_w2;
    const float *m1_b2;
    const float *m2_w1;     /* Adam's second moment */
    const float *m2_b1;
    const float *m2_w2;
    const float *m2_b2;
    float *child_w1;        /* [M S][D][H]   the children, written by sample */
    float *child_b1;        /* [M S][H] */
    float *child_w2;        /* [M S][H][MB] */
    float *child_b2;        /* [M S][MB] */
    float *new_w1;          /* the new mean, written by update and step */
    float *new_b1;
    float *new_w2;
    float *new_b2;
    float *new_sigma_w1;    /* the new sigma, written by update and step */
    float *new_sigma_b1;
    float *new_sigma_w2;
    float *new_sigma_b2;
    float *new_m1_w1;       /* the new moments, written by update and step with REM2D_SNES_ADAM */
    float *new_m1_b1;
    float *new_m1_w2;
    float *new_m1_b2;
    float *new_m2_w1;
    float *new_m2_b1;
    float *new_m2_w2;
    float *new_m2_b2;
    void *scratch;          /* scratch_bytes bytes, 8-byte aligned; NULL where rem2d_snes_scratch_bytes is 0 */
    uint64_t scratch_bytes; /* what `scratch` holds: at least rem2d_snes_scratch_bytes(e) */
} rem2d_snes;

/* REM2D_SNES_ABI_VERSION of the library */
int rem2d_snes_abi_version(void);

/* Bytes of scratch that rem2d_snes_update and rem2d_snes_step need for e (its shapes, n_means, group_size and pair_chunk; no
 * pointer is looked at), 0 where the pairs are not split; REM2D_E_INVALID (negative) for a NULL e, a dimension out of range (the
 * limits of rem2d_policy), n_means < 1, a group_size that is odd, below 2 or above REM2D_SNES_MAX_GROUP, n_means * group_size above
 * 2^31 - 1, a negative pair_chunk, an unknown bit in flags. */
int64_t rem2d_snes_scratch_bytes(const rem2d_snes *e);

/* The children of one generation: one kernel that reads every word of the mean and of sigma and writes every child word once.
 * REM2D_E_INVALID for what rem2d_snes_scratch_bytes refuses, a NULL mean, sigma or child pointer, a child buffer that overlaps a
 * buffer of the mean, of sigma or another child buffer.  Nothing else is looked at. */
int rem2d_snes_sample(const rem2d_snes *e, void *stream);

/* The new mean and state from the mean, the state and whatever e->util holds: one kernel, or two where the pairs are split.
 * REM2D_E_INVALID for what rem2d_snes_scratch_bytes refuses; a NULL util, mean, sigma, new-mean or new-sigma pointer, and with
 * REM2D_SNES_ADAM a NULL m1, m2, new-m1 or new-m2 pointer; an output that overlaps an input (util, mean, sigma, and with
 * REM2D_SNES_ADAM m1, m2) or another output; sigma_min / sigma_max that are not finite or not 0 < sigma_min <= sigma_max; a scratch
 * that is NULL, not 8-byte aligned or smaller than rem2d_snes_scratch_bytes(e) where that is not 0, or that overlaps an input or
 * an output.  fitness and the children are not looked at. */
int rem2d_snes_update(const rem2d_snes *e, void *stream);

/* The ES shape call on fitness into util, then rem2d_snes_update: two or three launches queued by one call.  REM2D_E_INVALID
 * also for a NULL fitness.  Everything is checked before the first launch. */
int rem2d_snes_step(const rem2d_snes *e, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_SNES_H */
