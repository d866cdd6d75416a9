#ifndef REM2D_OBSNORM_H
#define REM2D_OBSNORM_H

/* Observation normalisation for device policies in librem2d.so: running mean / standard deviation of a policy's input words, kept
 * on the device in EXACT integer sums, and applied inside the forward pass where a row is staged -- ARS's "V2" (Mania et al. 2018),
 * OpenAI-ES's virtual batch normalisation.  A header of its own: nothing here changes what a step, an observation row, a ray
 * fraction, the plain forward passes or any search operator hold, or any other ABI version.  The CPU twin has no counterpart of
 * anything in this header.
 *
 * Conventions.  A block is `group_size` = S consecutive population rows, as in the evolution-strategy header: row r belongs to block
 * r / S.  The last block may be partial; a call on n_rows rows wants n_rows <= n_blocks S.  Dn = 8 + 6 MB + R is the number of
 * normalised words of a row: the observation row, then the R ray fractions.  The K context words of a policy with memory are NOT
 * normalised and have no statistics.
 *
 * ---- 1. The state (caller-owned int64 words, exact) ----
 * Per block b: count[b] = n.  Per (block, word): s1[b][i], s2hi[b][i], s2lo[b][i].  A row CONTRIBUTES iff row_mask == NULL or its
 * row_mask byte is non-zero, AND all Dn of its words are finite: a row with a NaN or an infinite word contributes nothing to any
 * word.  For a contributing row and each word x:
 *   c = x < -2048.0f ? -2048.0f : (x > 2048.0f ? 2048.0f : x)
 *   q = (int64) rintf(c * 4096.0f)          the product is exact; ties to even; |q| <= 2^23 (-0 and the subnormals give 0)
 *   s1 += q;   p = q q;   s2hi += p >> 23;   s2lo += p & (2^23 - 1);   and n += 1 once per row
 * All sums are integers: they are the same bits whatever the launch shape (`row_chunk`), the order of the atomic additions or the
 * build, and two calls add up to what one call on the concatenation gives.  With n <= 2^39 contributing rows per block -- the
 * lifetime capacity of a block -- |s1|, s2hi and s2lo are at most 2^62.  KEEPING BELOW 2^39 ROWS PER BLOCK IS THE CALLER'S DUTY; the
 * library does not look.
 *
 * ---- 2. The accumulation (rem2d_obsnorm_accumulate) ----
 * One launch over obs[n_rows][8 + 6 MB] and frac[n_rows][R], the two arrays a policy descriptor names.  The lanes of a wavefront
 * run over the words of a row, so a row is one coalesced read; a wavefront takes `row_chunk` consecutive rows of ONE block, votes
 * on each row's finiteness inside the wavefront and sums its rows in registers; the wavefronts of a workgroup that hold the same
 * block add up in LDS; then 64-bit integer atomic additions to the state.  No floating-point atomics.  n_rows == 0 launches
 * nothing.
 *
 * ---- 3. The tables (rem2d_obsnorm_freeze) ----
 * One thread per (block, word) turns the state into mu[n_blocks][Dn] and inv[n_blocks][Dn], binary32.  Binary64 where a double
 * stands, each operation separately and correctly rounded, nothing fused in any build of the library:
 *   n < min_count:   mu = 0.0f,  inv = 1.0f                                  (the identity)
 *   else  nd = (double)n;   m = (double)s1 / nd
 *         s2 = ((double)s2hi * 8388608.0 + (double)s2lo) / nd
 *         v  = s2 - (m * m);   if !(v > 0) v = 0
 *         mu = (float)(m / 4096.0);   vx = (float)(v / 16777216.0)
 *         inv = vx >= min_var ? 1.0f / sqrtf(vx) : 0.0f
 * sqrtf and the binary32 quotient are the correctly rounded ones.  inv = 0 switches a word off that (almost) never varies: a body
 * count within a morphology, the words of an empty body slot.
 *
 * ---- 4. The application, inside the forward pass ----
 * Where the kernel stages word i < Dn of row r of block b = r / S, it stages
 *   d = x - mu[b][i];   t = d * inv[b][i];   x^ = t > clip ? clip : (t < -clip ? -clip : t)
 * two separately rounded binary32 operations and two comparisons, never fused, in any build; clip > 0 may be +inf; a NaN stays a NaN
 * (inf * 0 is one) and ends as valid = 0.  obs and frac keep their raw values and there is no extra pass over them.
 * THE LAW: targets, valid and -- with memory -- the context words are the bits the plain forward pass of the policy header (with
 * memory: of the header of policies with memory) writes when fed x^ as its obs / frac.  With mu = +0, inv = 1 and clip = +inf the
 * bits are the plain pass's own: x - 0 and x * 1 return x for every x, -0 included.
 *
 * ---- 5. The stream ----
 * The calls take no stream parameter: the stream is the descriptor's `stream` field, as rem2d_step_group's is.  The contract is the
 * one of every stream-taking function of the library all the same: all work is queued on that stream (NULL: the default stream) on
 * the device that is current, nothing synchronises, the library allocates nothing; tests/test_obsnorm_gpu.py holds the five calls to
 * it, under a capture and behind a gate.  They stand outside the table of tests/caller_stream.py only because that table could not
 * be extended when they were added; moving them into it (a `void *stream` parameter and five rows) is a follow-up.
 *
 * A host model reproduces every bit (tests/obsnorm_model.py). */

#include "rem2d_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_OBSNORM_ABI_VERSION 1
#define REM2D_OBSNORM_MAX_CHUNK 65536     /* row_chunk */
#define REM2D_OBSNORM_CAPACITY_LOG2 39    /* contributing rows per block over a state's lifetime: at most 2^39 */

/* Caller-owned device pointers and the shapes they have. */
typedef struct rem2d_obsnorm {
    int32_t max_bodies;      /* MB: 1 .. 64 */
    int32_t n_rays;          /* R: 0 .. 64;  Dn = 8 + 6 MB + R */
    int32_t n_blocks;        /* M >= 1 */
    int32_t group_size;      /* S >= 1 rows per block, M S <= 2^31 - 1 */
    int32_t row_chunk;       /* the launch shape of the accumulation: 0 = the library chooses, 1 .. 65536 = rows of a block that one
                                wavefront sums.  No result depends on it */
    int32_t context;         /* K: 0 = a feed-forward policy; >= 1: the policy carries K context words in `memory` (forward_memory, and
                                act_normed takes the pass with memory) */
    float clip;              /* > 0, may be +inf: forward and act */
    float min_var;           /* > 0, finite: freeze */
    int64_t min_count;       /* >= 1: freeze */
    int64_t n_rows;          /* N >= 0, N <= M S: the rows of accumulate; not looked at by the other calls */
    const float *obs;        /* [N][8 + 6 MB]: accumulate */
    const float *frac;       /* [N][R]; may be NULL when R == 0: accumulate */
    const uint8_t *row_mask; /* [N] or NULL: accumulate */
    int64_t *count;          /* [M]      the state: accumulate adds, freeze reads */
    int64_t *s1;             /* [M][Dn] */
    int64_t *s2hi;           /* [M][Dn] */
    int64_t *s2lo;           /* [M][Dn] */
    float *mu;               /* [M][Dn]  the tables: freeze writes, forward and act read */
    float *inv;              /* [M][Dn] */
    float *memory;           /* [rows][K], read and written in place where context >= 1; else not looked at */
    const uint8_t *reset;    /* [rows] or NULL where context >= 1: non-zero = this row's context reads as +0.0f */
    int64_t reserved;        /* 0 */
    void *stream;            /* the hipStream_t all work is queued on; NULL: the default stream (section 5) */
} rem2d_obsnorm;

/* REM2D_OBSNORM_ABI_VERSION of the library */
int rem2d_obsnorm_abi_version(void);

/* The accumulation (section 2).  REM2D_E_INVALID for a NULL descriptor, a max_bodies or n_rays out of range, n_blocks < 1,
 * group_size < 1, M S or M Dn above 2^31 - 1, row_chunk outside 0 .. 65536, a non-zero reserved, n_rows < 0, n_rows > M S, a NULL obs,
 * frac (with R > 0), count, s1, s2hi or s2lo, a state array that is not 8-byte aligned.  Nothing else is looked at.  Everything is
 * checked before the launch; nothing is written after a refusal. */
int rem2d_obsnorm_accumulate(const rem2d_obsnorm *n);

/* The tables (section 3).  REM2D_E_INVALID for what the accumulation refuses of the shapes, a min_count < 1, a min_var that is
 * not positive and finite, a NULL count, s1, s2hi, s2lo, mu or inv, a state array that is not 8-byte aligned.  n_rows, obs, frac,
 * row_mask, clip and context are not looked at. */
int rem2d_obsnorm_freeze(const rem2d_obsnorm *n);

/* The normalised forward pass of a feed-forward policy (section 4): rem2d_policy_forward's kernel with the application in its
 * staging, one launch.  REM2D_E_INVALID for what rem2d_policy_forward refuses of p, what the accumulation refuses of the shapes,
 * p->max_bodies != max_bodies, p->n_rays != n_rays, p->n_rows > M S, a clip that is not > 0 (a NaN included), a NULL mu or inv, a
 * context other than 0. */
int rem2d_obsnorm_forward(const rem2d_obsnorm *n, const rem2d_policy *p);

/* The same for a policy with memory: the kernel of the header of policies with memory with the application in its staging.  p is
 * that header's `p` member -- p->d == 8 + 6 MB + R + K --, and context, memory and reset are that header's members of the same
 * names.  REM2D_E_INVALID for what that header's forward call refuses of them, and for what rem2d_obsnorm_forward refuses
 * otherwise. */
int rem2d_obsnorm_forward_memory(const rem2d_obsnorm *n, const rem2d_policy *p);

/* One control step of a population under a normaliser: rem2d_worlds_observe into p->obs, rem2d_worlds_sense into p->frac if
 * n_rays > 0, with `accumulate` != 0 the accumulation of those two arrays under p->row_mask over p->n_rows rows (the descriptor's
 * own obs, frac, row_mask and n_rows are not looked at), the normalised forward pass -- rem2d_obsnorm_forward where context == 0,
 * rem2d_obsnorm_forward_memory otherwise -- and rem2d_worlds_control with p->targets / p->valid: as many launches as
 * rem2d_worlds_act, plus one when accumulating, all on the descriptor's stream.  The tables are read as they stand: what this
 * call accumulates shows after the next rem2d_obsnorm_freeze.  Everything is checked before the first launch: what the forward
 * call and (when accumulating) the accumulation refuse, and what rem2d_worlds_act refuses of its worlds and ray offsets. */
int rem2d_worlds_act_normed(rem2d_world *const *worlds, int32_t n_worlds, const rem2d_obsnorm *n, const rem2d_policy *p,
                            const double *ray_offsets_dev, int32_t accumulate);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_OBSNORM_H */
