#ifndef REM2D_ELITES_H
#define REM2D_ELITES_H

/* MAP-Elites for device policies in librem2d.so: per morphology a grid over behaviour space whose every cell keeps the best weight
 * set ever seen there, the insertion of a whole evaluated population into it, and the emission of mutated copies of uniformly drawn
 * elites.  A header of its own, like rem2d_evolve.h, the evolution-strategy header and the novelty header: nothing here changes
 * what a step, an observation row, a forward pass or an older search operator holds.  The CPU twin has no counterpart of anything
 * in this header.
 *
 * ---- 1. The grid (state the caller owns) ----
 * Rows: desc[G][B] (binary32, B = width words, as the novelty header lays descriptors out), fitness[G] (binary64) and G weight sets
 * w1[D][H], b1[H], w2[H][MB], b2[MB] as rem2d_policy.h lays sets out; row c belongs to set c.  The rows form M = n_blocks blocks
 * of S = group_size consecutive rows, G = M S; a block is one morphology.  All blocks share one cell map of n_dims dimensions;
 * dimension i looks at word[i] of a row and has bins[i] cells, C = bins[0] * ... * bins[n_dims - 1] cells in all.  Per block b and
 * cell q the grid holds
 *   elite_fitness[M][C] (binary64), elite_desc[M][C][B], count[M][C] (int32: the replacements the cell has seen; a cell is EMPTY
 *   iff its count is 0) and the four weight arrays elite_w1[M C][D][H], elite_b1, elite_w2, elite_b2: slot b C + q is one set.
 * The cell of a row, for every dimension i:
 *   x = the row's word word[i];  u = (x - lo[i]) * inv[i]     the difference and the product one correctly rounded binary32
 *                                                             operation each, in any build of the library
 *   q_i = 0 if u < 0;  q_i = bins[i] - 1 if u >= (float)bins[i];  otherwise q_i = (int)u (truncation)
 *   cell = q_0 stride_0 + q_1 stride_1 + ...,  stride_0 = 1, stride_i = stride_{i-1} bins[i-1]
 * so behaviour outside [lo, hi) lands in the border cells.  The caller computes inv[i] = (float)bins[i] / ((float)hi - (float)lo)
 * in binary32.  A row is ADMISSIBLE iff every selected word is finite, its fitness is not a NaN (+-inf are fitness values) and
 * mask == NULL or mask[c] != 0.
 *
 * ---- 2. The insertion (rem2d_elites_insert) ----
 * Writes cell[G]: the cell of every admissible row, -1 for the others.  The candidates of (b, q) are the admissible rows of block b
 * whose cell is q.  The CHALLENGER is the candidate of greatest fitness in the order of rem2d_evolve.h (-0 == +0), ties to the
 * LOWEST row.  It replaces the incumbent iff the cell is empty or its fitness is STRICTLY greater than elite_fitness[b][q] (an
 * incumbent NaN is below everything).  On a replacement by row w:
 *   elite_fitness[b][q] = fitness[w]'s bits;  elite_desc[b][q] = desc[w]'s bits;  the four arrays of slot b C + q = the bits of set
 *   w;  count[b][q] += 1;  winner[b][q] = w.
 * Everything else of the grid is untouched and winner[b][q] = -1 there.  The result is a function of the inputs alone: no float
 * atomics, nothing that depends on the order in which rows are looked at.
 * Example (M = 1, S = 4, B = 1, one dimension: word 0, lo 0, inv 1, 4 bins; the grid empty but for cell 3 with fitness 9):
 *   desc = [0.5, 0.25, 2.0, 7.0], fitness = [1, 1, -0.0, 5]
 *   cell = [0, 0, 2, 3] (7.0 is clamped into the last cell);  the tie in cell 0 goes to row 0;  the incumbent of cell 3 holds
 *   winner = [0, -1, 2, -1];  count: cells 0 and 2 go from 0 to 1;  inserting the same rows again changes nothing: winner = -1
 *   everywhere, since equal fitness does not replace.
 *
 * ---- 3. The emission (rem2d_elites_sample, rem2d_elites_emit) ----
 * n_children = M S' children, S' = n_children / M consecutive children per block.  Let f_0 < ... < f_{n-1} be the filled cells of
 * block b; n_filled[b] = n.  For child c of block b, x0 is the first output word of Philox4x32-10 exactly as rem2d_evolve.h states
 * it (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds), key = (seed & 0xffffffff,
 * seed >> 32), counter = (0, c, generation, 10): domain 10, disjoint from the domains 0 .. 9 of the three search headers.
 *   j = ((uint64)x0 * n) >> 32;  parent[c] = b C + f_j;  for n = 0: parent[c] = -1.
 * rem2d_elites_sample is that draw alone.  rem2d_elites_emit then writes child set c from slot parent[c] of the elite arrays exactly
 * as rem2d_evolve.h states the variation with elite = 0: per element the counter (i, c, generation, domain 1 .. 4), a miss copies
 * the bits, a hit adds sigma * z; a child whose parent is -1 keeps the words it holds.
 * Example: a block with cells 1 and 5 filled of C = 8: n = 2, a child with x0 < 2^31 descends from cell 1, the others from cell 5;
 *          a block with no filled cell: n_filled = 0, every parent -1, its children's words stay as they are.
 *
 * A host model reproduces every bit (tests/elites_model.py).  The library allocates nothing; every call is asynchronous on `stream`,
 * on the device that is current.  Scratch: rem2d_elites_scratch_bytes of caller-owned device memory, cleared by the calls
 * themselves; what it holds between calls means nothing. */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_ELITES_ABI_VERSION 1
#define REM2D_ELITES_MAX_WIDTH 32     /* B */
#define REM2D_ELITES_MAX_DIMS 4       /* n_dims */
#define REM2D_ELITES_MAX_CELLS 65536  /* C */

/* Caller-owned device pointers and the shapes they have. */
typedef struct rem2d_elites {
    int32_t d;               /* D: input rows of w1, 8 + 6 max_bodies + R with R in 0 .. 64 */
    int32_t hidden;          /* H: 1 .. 128 */
    int32_t max_bodies;      /* MB: 1 .. 64 */
    int32_t width;           /* B: 1 .. 32 */
    int32_t n_blocks;        /* M >= 1 */
    int32_t group_size;      /* S >= 1 rows per block: insert looks at G = M S rows; not looked at by sample and emit */
    int32_t n_children;      /* M S', a positive multiple of M: sample and emit; not looked at by insert */
    int32_t n_dims;          /* 1 .. 4 */
    int32_t word[4];         /* per dimension: 0 .. B - 1; entries at and beyond n_dims are not looked at */
    int32_t bins[4];         /* >= 1, their product C <= 65536 and M C <= 2^31 - 1 */
    float lo[4];             /* finite */
    float inv[4];            /* finite, > 0 */
    uint32_t generation;     /* counter word 2 of the draw and the mutation */
    float sigma;             /* mutation step */
    uint64_t rate_threshold; /* floor(rate * 2^32): 0 .. 2^32 */
    uint64_t seed;           /* the Philox key */
    const float *desc;       /* [G][B]; read by insert; may not overlap a grid buffer */
    const double *fitness;   /* [G]; read by insert */
    const uint8_t *mask;     /* [G] or NULL; read by insert */
    const float *w1;         /* [G][D][H]   the evaluated sets; read by insert; none may overlap an elite weight buffer */
    const float *b1;         /* [G][H] */
    const float *w2;         /* [G][H][MB] */
    const float *b2;         /* [G][MB] */
    double *elite_fitness;   /* [M][C]      the grid: read and written by insert */
    float *elite_desc;       /* [M][C][B] */
    float *elite_w1;         /* [M C][D][H] read by emit */
    float *elite_b1;         /* [M C][H] */
    float *elite_w2;         /* [M C][H][MB] */
    float *elite_b2;         /* [M C][MB] */
    int32_t *count;          /* [M][C]; read by sample and emit */
    int32_t *cell;           /* [G]; written by insert */
    int32_t *winner;         /* [M][C]; written by insert */
    float *child_w1;         /* [M S'][D][H]  written by emit; none may overlap an elite weight buffer */
    float *child_b1;         /* [M S'][H] */
    float *child_w2;         /* [M S'][H][MB] */
    float *child_b2;         /* [M S'][MB] */
    int32_t *parent;         /* [M S']; written by sample and emit */
    int32_t *n_filled;       /* [M]; written by sample and emit */
    void *scratch;           /* rem2d_elites_scratch_bytes bytes, 8-byte aligned: all three calls */
    uint64_t scratch_bytes;  /* what `scratch` holds */
    int32_t reserved;        /* 0 */
} rem2d_elites;

/* REM2D_ELITES_ABI_VERSION of the library */
int rem2d_elites_abi_version(void);

/* Bytes of scratch the calls need for these shapes (12 M C), or REM2D_E_INVALID (negative) for a NULL e, a dimension out of range,
 * n_blocks < 1, n_dims outside 1 .. 4, a word outside [0, B), bins < 1, more than 65536 cells, M C above 2^31 - 1, a lo or inv that
 * is not finite, an inv that is not positive, a rate_threshold above 2^32, a non-zero reserved.  No pointer is looked at. */
int64_t rem2d_elites_scratch_bytes(const rem2d_elites *e);

/* The insertion: four launches (clear, the per-cell maximum, the lowest row that has it, the commit).  REM2D_E_INVALID for what
 * rem2d_elites_scratch_bytes refuses, a group_size < 1 or M S above 2^31 - 1, a NULL desc, fitness, weight, grid, cell, winner or
 * scratch pointer, a scratch that is misaligned or too small, a desc that overlaps a grid buffer, an evaluated weight buffer that
 * overlaps an elite weight buffer.  The child buffers, parent and n_filled are not looked at. */
int rem2d_elites_insert(const rem2d_elites *e, void *stream);

/* The draw alone: n_filled[M] and parent[M S'], one launch.  REM2D_E_INVALID for what rem2d_elites_scratch_bytes refuses, an
 * n_children that is not a positive multiple of n_blocks, a NULL count, parent, n_filled or scratch pointer, a scratch that is
 * misaligned or too small.  Nothing else is looked at. */
int rem2d_elites_sample(const rem2d_elites *e, void *stream);

/* rem2d_elites_sample, then the variation of rem2d_evolve.h from the elite arrays: two launches queued by one call.
 * REM2D_E_INVALID as rem2d_elites_sample, and for a NULL elite or child weight pointer and a child buffer that overlaps an elite
 * weight buffer.  Everything is checked before the first launch. */
int rem2d_elites_emit(const rem2d_elites *e, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_ELITES_H */
