#ifndef REM2D_EVOLVE_H
#define REM2D_EVOLVE_H

/* Evolving device policies for librem2d.so: tournament selection and Gaussian-like mutation of the weight sets of
 * include/rem2d_policy.h, for a WHOLE population, on the device -- the variation step of the reference's generation loop
 * (select -> clone -> mutate -> evaluate, REM2D_main.py:280-298) between two episodes.  A header of its own, like rem2d_policy.h:
 * nothing here changes what a step, an observation row or a forward pass holds.
 *
 * The population is data: G weight sets w1[D][H], b1[H], w2[H][MB], b2[MB] (binary32, as rem2d_policy lays them out) and one
 * binary64 fitness per set, in device memory the caller owns.  The children are written into four other buffers of the same shapes.
 *
 * Random stream: Philox4x32-10 as Random123 defines it -- multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 * 0xBB67AE85, ten rounds.  key = (seed & 0xffffffff, seed >> 32); counter = (i, c, generation, domain), c the child set, domain 0 for
 * selection and 1, 2, 3, 4 for w1, b1, w2, b2, i = 0 for selection and otherwise the element's index inside that array of ONE set.
 * The four output words are x0 .. x3.  Every draw is a function of (seed, generation, c, domain, i) alone: no state, no order.
 *
 * Selection writes parent[G].  The sets form blocks of S = group_size consecutive sets (S divides G; S = G: one population; creatures
 * that share a morphology are the caller's blocks).  Order on fitness: every NaN equals every other NaN and is below everything
 * else; -0 == +0; otherwise the usual order.  For child c, base = (c / S) S:
 *   elite == 1 and c == base:  parent[c] = the lowest index of the block whose fitness is maximal.
 *   otherwise, T = tournsize:  aspirant a_k = base + (((uint64)x_k * S) >> 32), k < T; the winner starts as a_0 and a_k replaces it
 *                              only if STRICTLY greater (deap's selTournament, ties to the earlier aspirant).
 *
 * Variation writes child set c from set p = parent[c]; a p outside [0, G) leaves the words of child c untouched.  For every element
 * w of every array of p, with x0 .. x3 of its counter:
 *   elite == 1 and c == base:         the child's word is w's bits.
 *   (uint64)x0 >= rate_threshold:     a miss: w's bits (NaN payloads, infinities, denormals and signed zeros pass unchanged).
 *   otherwise a hit:                  w + (sigma * z),  z = (float)s * C,
 *                                     s = the sum of the six 16-bit halves of x1, x2, x3, minus 196605 (an int32, exact in
 *                                     binary32), C = the binary32 constant 0x37B504F3 (fl32(sqrt 2) * 2^-16): an Irwin-Hall sum of
 *                                     six, unit variance, support +-4.24.
 * rate_threshold = floor(rate * 2^32), computed by the caller, in [0, 2^32]: 0 hits nothing, 2^32 everything.  The conversion, the
 * two products and the sum are one correctly rounded binary32 operation each, nothing is fused, in any build of the library, and
 * there is no transcendental function: a host model reproduces every bit (tests/evolve_model.py).  Where a hit produces a NaN (a NaN
 * parent word, inf * 0, inf - inf) its sign and payload are undefined, as IEEE 754 leaves them.
 *
 * The library allocates nothing; all three calls are asynchronous on `stream`, on the device that is current. */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_EVOLVE_ABI_VERSION 1
#define REM2D_EVOLVE_MAX_TOURNSIZE 4

/* Caller-owned device pointers and the shapes they have. */
typedef struct rem2d_evolve {
    int32_t d;               /* D: input rows of w1, 8 + 6 max_bodies + R with R in 0 .. 64 (REM2D_SENSE_MAX_RAYS) */
    int32_t hidden;          /* H: 1 .. 128 (REM2D_POLICY_MAX_HIDDEN) */
    int32_t max_bodies;      /* MB: 1 .. 64 (REM2D_CONTROL_MAX_BODIES) */
    int32_t n_sets;          /* G >= 1 weight sets, parents and children alike */
    int32_t group_size;      /* S >= 1, a divisor of G */
    int32_t tournsize;       /* T: 1 .. REM2D_EVOLVE_MAX_TOURNSIZE */
    int32_t elite;           /* 0 | 1: the first child of every block is the block's best set, unmutated */
    uint32_t generation;     /* counter word 2 */
    uint64_t rate_threshold; /* floor(rate * 2^32): 0 .. 2^32 */
    uint64_t seed;           /* the Philox key */
    float sigma;             /* mutation step */
    int32_t reserved;        /* 0 */
    const double *fitness;   /* [G]; read by select and evolve */
    const float *w1;         /* [G][D][H]   the parents */
    const float *b1;         /* [G][H] */
    const float *w2;         /* [G][H][MB] */
    const float *b2;         /* [G][MB] */
    float *child_w1;         /* [G][D][H]   the children, written by vary and evolve; none may overlap a parent buffer */
    float *child_b1;         /* [G][H] */
    float *child_w2;         /* [G][H][MB] */
    float *child_b2;         /* [G][MB] */
    int32_t *parent;         /* [G]; written by select and evolve, read by vary */
} rem2d_evolve;

/* REM2D_EVOLVE_ABI_VERSION of the library */
int rem2d_evolve_abi_version(void);

/* Selection alone: parent[c] for every child, one kernel.  REM2D_E_INVALID for a NULL e, fitness or parent, a dimension out of
 * range (the limits of rem2d_policy), n_sets < 1, a group_size < 1 or that does not divide n_sets, a tournsize outside 1 .. 4, an
 * elite outside {0, 1}, a rate_threshold above 2^32.  The weight pointers are not looked at. */
int rem2d_policy_select(const rem2d_evolve *e, void *stream);

/* Variation alone, from whatever e->parent holds (the caller may have filled it): one kernel that reads every parent word once
 * and writes every child word once.  REM2D_E_INVALID for what rem2d_policy_select refuses about shapes and parameters, a NULL
 * parent, a NULL weight pointer, and a child buffer that overlaps a parent buffer.  fitness is not looked at. */
int rem2d_policy_vary(const rem2d_evolve *e, void *stream);

/* rem2d_policy_select, then rem2d_policy_vary: two launches queued by one call.  Everything is checked before the first. */
int rem2d_policy_evolve(const rem2d_evolve *e, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_EVOLVE_H */
