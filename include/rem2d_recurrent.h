#ifndef REM2D_RECURRENT_H
#define REM2D_RECURRENT_H

/* Recurrent device policies for librem2d.so: the controller of include/rem2d_policy.h with MEMORY -- an Elman-style partially
 * recurrent network whose first K hidden activations of one control step are K extra input words of the next.  The K context
 * words of every population row live in device memory the caller owns and are read and rewritten in place by one kernel that
 * evaluates the whole population.  A header of its own: nothing here changes what rem2d_policy_forward computes, what a step,
 * an observation row or a ray fraction holds, or any other ABI version.
 *
 * For population row r with weight set g (resolved as rem2d_policy.h states: index[r], or r), MB = p.max_bodies, R = p.n_rays
 * and K = context:
 *
 *   context  c_k  = reset && reset[r] ? +0.0f : memory[r][k]          (a substitution, not a product: a NaN in memory does
 *                                                                       not survive a reset)
 *   input    x    = the D = 8 + 6 MB + R + K binary32 words: the observation row, then the R ray fractions, then c_0 .. c_{K-1}
 *   a_j, h_j, y_m, t_m, targets[r][m], valid[r][m]: exactly as rem2d_policy.h states them, over these D words in ascending
 *                   order, with w1[D][H] -- the K last rows of w1 are the recurrent weights
 *   memory   memory[r][k] = h_k for k < K, stored as computed, non-finite values included
 *
 * The arithmetic rules are those of rem2d_policy.h: every product, sum and quotient is one separately, correctly rounded binary32
 * operation, nothing is fused in any build of the library, and there is no transcendental function (tests/recurrent_model.py
 * reproduces every bit).  A row that the row mask clears, or whose index names no weight set, is skipped entirely: its targets,
 * its valid bytes AND its memory stay as they are.
 *
 * The law that follows: `targets` and `valid` are the bits rem2d_policy_forward writes for the same weights with
 * n_rays = R + K and frac' = [frac | c].  A recurrent weight set is, to anything that only moves weights about, an ordinary set
 * with d = 8 + 6 MB + (R + K); that is why R + K is held to the 64 "ray" inputs a feed-forward set may have.
 *
 * In place: a row belongs to exactly one wavefront, which reads the row's K context words before it writes any of them; no
 * other row's memory is read.  The library allocates nothing. */

#include "rem2d_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_RECURRENT_ABI_VERSION 1

/* Caller-owned device pointers and the shapes they have. */
typedef struct rem2d_recurrent {
    rem2d_policy p;        /* as for rem2d_policy_forward, except: p.d == 8 + 6 * p.max_bodies + p.n_rays + context */
    int32_t context;       /* K: 1 .. min(p.hidden, 64 - p.n_rays) */
    int32_t reserved;      /* 0 */
    float *memory;         /* [n_rows][K], read and written in place */
    const uint8_t *reset;  /* [n_rows] or NULL: non-zero = this row's context reads as +0.0f */
} rem2d_recurrent;

/* REM2D_RECURRENT_ABI_VERSION of the library */
int rem2d_recurrent_abi_version(void);

/* The recurrent forward pass alone, on whatever the rows of q->p.obs / q->p.frac and q->memory hold: one kernel on `stream`,
 * asynchronous, on the device that is current.  REM2D_E_INVALID for a NULL q or a NULL memory, context < 1, context > p.hidden,
 * p.n_rays + context > 64, p.d != 8 + 6 p.max_bodies + p.n_rays + context, reserved != 0, and everything rem2d_policy_forward
 * refuses of p (its rule for d replaced by the one above). */
int rem2d_recurrent_forward(const rem2d_recurrent *q, void *stream);

/* rem2d_worlds_act with the recurrent pass in the middle: rem2d_worlds_observe into q->p.obs, rem2d_worlds_sense into q->p.frac
 * if p.n_rays > 0, the recurrent forward pass, and rem2d_worlds_control with q->p.targets / q->p.valid.  The same number of
 * launches as rem2d_worlds_act.  Everything is checked before the first launch: what rem2d_recurrent_forward refuses and what
 * rem2d_worlds_act refuses of its worlds and ray offsets. */
int rem2d_worlds_act_recurrent(rem2d_world *const *worlds, int32_t n_worlds, const rem2d_recurrent *q, const double *ray_offsets_dev,
                               void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_RECURRENT_H */
