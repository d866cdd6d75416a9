#ifndef REM2D_PARETO_H
#define REM2D_PARETO_H

/* Pareto ranking for librem2d.so: the non-dominated fronts, the crowding distance and a rank utility of rows of several objectives
 * (what NSGA-II orders a population by), and the local-competition score of novelty search with local competition (Lehman and
 * Stanley): among a row's nearest behavioural neighbours, how many it out-performs.  A header of its own, like every search
 * operator before it: nothing here changes what a step, an observation row, a forward pass or another operator holds.  The CPU
 * twin has no counterpart of anything in this header.
 *
 * Both calls work on G = n_rows rows in M = G / S blocks of S = group_size consecutive rows; everything below is per block, and no
 * result depends on the launch shape.
 *
 * ---- 1. The rank (rem2d_pareto_rank) ----
 * obj[G][K] (binary64), K = n_obj in 1 .. 4, every objective maximised.
 *   admitted:   a row is admitted iff all K of its words are finite.
 *   domination: row i dominates row j iff both are admitted, obj[i][m] >= obj[j][m] for every m, and > for some m (binary64
 *               compares: -0 equals +0).
 *   front:      front[c] = 0 for an admitted row that nobody dominates, else 1 + the greatest front among its dominators (the
 *               peel).  F = the number of admitted fronts (0 where no row is admitted).  An unadmitted row gets front = F.
 *   crowding:   value-based, so it depends on no sort's stability.  For an admitted row c and every m, ascending:  v = obj[c][m];
 *               below = the greatest value strictly less than v, above = the least value strictly greater than v, lo and hi the
 *               least and the greatest value, all four of objective m among the rows of c's front.  If below or above does not
 *               exist for any m:  crowd[c] = +inf.  Otherwise
 *                   crowd = 0.0;  for m = 0 .. K - 1 ascending:  crowd = crowd + ((above - below) / (hi - lo))
 *               every subtraction, division and sum one correctly rounded binary64 operation; an overflow or inf / inf gives what
 *               IEEE 754 gives (a NaN has no defined sign or payload).  Rows with identical objective vectors therefore get
 *               identical crowding.  An unadmitted row gets crowd = 0.0.
 *   order:      row c is better than row j iff front[c] < front[j], or the fronts are equal and crowd[c] > crowd[j], a NaN crowd
 *               counting as below every number and equal to another NaN.
 *   utility:    util[c] = 2 L + E - (S - 1), L the number of other rows of the block that c is better than, E the number of other
 *               rows that are neither better nor worse: integers in -(S - 1) .. S - 1 whose sum over a block is 0.
 * This is the formula and the range of the evolution-strategy header's rank shaping, and with K = 1 and input that is finite or
 * NaN the result equals that shaping bit for bit: the fronts are the distinct values from the greatest down, every row of a front
 * holds the same value and so crowd = +inf, and the NaN rows share the last front.  (An infinite word is unadmitted here and ranks
 * with the NaNs; the shaping ranks it as a number.)
 * Outputs: front int32 [G], crowd binary64 [G], util int32 [G], n_fronts int32 [M] = F.  Each may be NULL and is then not written.
 * Example (K = 2, S = 6):  rows (1,5) (2,4) (3,3) (2,2) (1,1) (NaN,9)
 *   row   front  crowd  util
 *   0     0      inf     4        the first front is rows 0, 1, 2; its ends lack a neighbour on one side
 *   1     0      2       1        (3 - 1) / (3 - 1) + (5 - 3) / (5 - 3)
 *   2     0      inf     4
 *   3     1      inf    -1        alone in its front
 *   4     2      inf    -3
 *   5     3      0      -5        unadmitted: front = F = 3
 *   n_fronts = 3
 *
 * ---- 2. Local competition (rem2d_pareto_local) ----
 * desc[G][B] (binary32), B = width in 1 .. 32; fitness[G] (binary64); k in 1 .. 32.  Any S >= 1 that divides G.
 *   d2(x, y):   d2 = 0.0f;  for i = 0 .. B - 1 ascending:  t = x_i - y_i;  d2 = d2 + (t * t)
 *               every difference, product and sum one correctly rounded binary32 operation, nothing fused, in any build of the
 *               library (the arithmetic of the novelty header's score, restated).
 *   candidates: the OTHER rows of the block (c excluded by its index, not by its value) whose d2 to row c is finite.  No archive
 *               takes part.
 *   neighbours: the candidates in ascending order of (d2, row index); the first k' = min(k, the number of candidates) of them.
 *   local[c]    = (double) of the number of neighbours j whose fitness[j] is below fitness[c] in the evolve header's order on
 *               fitness: a NaN is below every number, a NaN is not below a NaN, equal is not below.  0.0 for k' = 0.  A row c with
 *               a non-finite descriptor word gets a NaN (sign and payload undefined); the rank then puts it in the last front.
 *   neighbours[c] int32 = k'.  The pointer may be NULL.
 * Example (B = 1, S = 4, k = 2):  desc = [0, 3, 4, 8], fitness = [5, 1, 7, 7]  ->  local = [1, 0, 2, 1]
 *   row 2 is at d2 = 16 from rows 0 and 3: the lower index wins and row 2 beats both its neighbours (1 and 0); the other choice
 *   would give 1.
 *
 * A host model reproduces every bit (tests/pareto_model.py).  The library allocates nothing; both calls are asynchronous on
 * `stream`, on the device that is current, and check everything before anything is dereferenced or launched. */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_PARETO_ABI_VERSION 1
#define REM2D_PARETO_MAX_OBJ 4      /* K */
#define REM2D_PARETO_MAX_GROUP 1024 /* S of the rank */
#define REM2D_PARETO_MAX_WIDTH 32   /* B */
#define REM2D_PARETO_MAX_K 32       /* k */

/* Caller-owned device pointers and the shapes they have.  Each call looks only at the members named for it. */
typedef struct rem2d_pareto {
    int32_t n_rows;        /* G >= 1 */
    int32_t group_size;    /* S >= 1, dividing G; rank: at most 1024 */
    int32_t n_obj;         /* rank: K, 1 .. 4 */
    int32_t width;         /* local: B, 1 .. 32 */
    int32_t k;             /* local: neighbours, 1 .. 32 */
    int32_t reserved;      /* 0 */
    const double *obj;     /* rank: [G][K], read */
    int32_t *front;        /* rank: [G] or NULL */
    double *crowd;         /* rank: [G] or NULL */
    int32_t *util;         /* rank: [G] or NULL */
    int32_t *n_fronts;     /* rank: [M] or NULL */
    const float *desc;     /* local: [G][B], read */
    const double *fitness; /* local: [G], read */
    double *local;         /* local: [G] */
    int32_t *neighbours;   /* local: [G] or NULL */
} rem2d_pareto;

/* REM2D_PARETO_ABI_VERSION of the library */
int rem2d_pareto_abi_version(void);

/* front, crowd, util and n_fronts of every block: one kernel.  REM2D_E_INVALID for a NULL descriptor, n_rows < 1, a group_size
 * outside 1 .. 1024 or not dividing n_rows, n_obj outside 1 .. 4, a non-zero reserved, a NULL obj, an output that overlaps obj. */
int rem2d_pareto_rank(const rem2d_pareto *p, void *stream);

/* local and neighbours of every row: one kernel.  REM2D_E_INVALID for a NULL descriptor, n_rows < 1, a group_size below 1 or not
 * dividing n_rows, width or k outside 1 .. 32, a non-zero reserved, a NULL desc, fitness or local, an output that overlaps desc or
 * fitness. */
int rem2d_pareto_local(const rem2d_pareto *p, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_PARETO_H */
