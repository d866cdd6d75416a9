#ifndef REM2D_CVT_H
#define REM2D_CVT_H

/* Centroid archives and the iso+line emitter for device policies in librem2d.so: CVT-MAP-Elites (Vassiliades et al. 2018) beside the
 * regular grids of the elite-grid header.  C centroids spread over the whole descriptor space replace the grid's cell map: a row
 * belongs to its NEAREST centroid.  The directional variation (Vassiliades & Mouret 2018) replaces blind mutation: a child is an
 * elite moved by isotropic noise and along the line to a second elite.  A header of its own, like the elite-grid header: nothing
 * here changes what a step, an observation row, a forward pass or an older search operator holds.  The CPU twin has no counterpart
 * of anything in this header.
 *
 * ---- 1. The archive (state the caller owns) ----
 * The grid state is the arrays of the elite-grid header's section 1 with the same meaning: elite_fitness[M][C] (binary64),
 * elite_desc[M][C][B], count[M][C] (a cell is EMPTY iff its count is 0), winner[M][C] and the four elite weight arrays, slot b C + q
 * one set.  To the grid header's sample and emit calls such an archive is a grid of one dimension with bins[0] = C: they look only
 * at count and the elite arrays.  New: centroids[C][B] (binary32), shared by all blocks; 1 <= C <= 65536, 1 <= B <= 32.
 *
 * The nearest centroid.  For row x and centroid y, d2(x, y) is exactly the novelty header's:
 *   d2 = 0.0f;  for i ascending: t = x_i - y_i;  d2 = d2 + (t * t)
 * each of the three one correctly rounded binary32 operation, never fused, in any build of the library, the -ffp-contract=fast one
 * included.  The cell of a row:
 *   best = -1, bestd = +inf;  for q = 0 .. C - 1 ascending: if d2(x, c_q) < bestd then best = q, bestd = d2
 * so that
 *   ties go to the LOWEST centroid;  a duplicate centroid never wins;
 *   a candidate whose d2 is a NaN or +inf is never chosen: a non-finite word in the row or in the centroid, an overflow;
 *   a row with no finite candidate has cell -1 and dist +inf.
 * Every finite d2 is >= +0, so its bit pattern orders as its value does: any split of the centroids over lanes, wavefronts or
 * workgroups that combines by the lexicographic minimum of (d2 bits, q) gives the same result.  The result does not depend on the
 * launch shape (`splits`).
 * Example (B = 1): centroids = [0, 2, 2, 10], rows = [1, 2, 7, NaN] give cell = [0, 1, 3, -1] and dist = [1, 0, 9, inf].
 *
 * ---- 2. The assignment (rem2d_cvt_assign) ----
 * cell[n_rows] and, where dist is not NULL, dist[n_rows] (the winning d2, +inf for cell -1) of desc[n_rows][B]: any n_rows rows, no
 * block structure, no fitness, no mask.  One launch, or three (clear, the split assign, the read-out) where the centroids are split
 * over workgroups: few rows and many centroids.
 *
 * ---- 3. The insertion (rem2d_cvt_insert) ----
 * The elite-grid header's section 2 verbatim, with "the cell of a row" replaced by the nearest centroid of the row, G = M S rows in
 * M blocks of S.  A row is ADMISSIBLE iff its cell is >= 0, its fitness is not a NaN (+-inf are fitness values) and mask == NULL or
 * mask[c] != 0; cell[c] = -1 for the others.  The challenger of (b, q) -- the admissible row of block b in cell q of greatest fitness
 * in the order of rem2d_evolve.h, ties to the LOWEST row --, the STRICT replacement, count, winner and the bit copies of fitness,
 * descriptor row and weight set are as the elites header states them.  dist, where not NULL, holds every row's d2 to its nearest
 * centroid, admissible or not.  The assignment's launches, then the elites' four (clear, key, row, commit).
 *
 * ---- 4. The line emission (rem2d_cvt_emit_line) ----
 * n_children = M S' children as in the elite-grid header's section 3.  Let f_0 < ... < f_{n-1} be the filled cells of block b;
 * n_filled[b] = n.  Philox4x32-10 and the key exactly as rem2d_evolve.h states them.  For child c of block b:
 *   parent[c]  is the grid header's sample draw, bit for bit: counter (0, c, generation, 10), j = ((uint64)x0 n) >> 32, b C + f_j
 *   parent2[c] = b C + f_j with j = ((uint64)x0 n) >> 32 from counter (0, c, generation, 11)
 *   a = sigma_line * zl (one binary32 product), zl the evolve header's z from x1 .. x3 of counter (0, c, generation, 12)
 * (domains 0 .. 10 are taken by the older headers; 11 and 12 are this one's.)  With x1, x2 the words of slots parent[c], parent2[c],
 * per element i of array k = 1 .. 4 (w1, b1, w2, b2):
 *   z from counter (i, c, generation, k) exactly as rem2d_evolve.h's variation takes it; EVERY element is hit, x0 is not looked at
 *   child = (x1 + (sigma_iso * z)) + (a * (x2 - x1))       five separate correctly rounded binary32 operations, in any build
 * If sigma_line is +-0 the second parent's words are not read and child = x1 + (sigma_iso * z): the grid header's emit at
 * rate_threshold = 2^32 and sigma = sigma_iso, bit for bit (parent2 is still written).  For n = 0 both parents are -1 and the child
 * keeps the words it holds.  n_filled[M] is written as the grid header's sample call writes it.  Two launches: the draw and the
 * variation.
 * The elite arrays may be those of a grid of the elite-grid header: only count, the elite weight arrays, M and C are looked at.
 *
 * ---- 5. The stream ----
 * The calls take no stream parameter: the stream is the descriptor's `stream` field, as rem2d_step_group's is.  The contract is the
 * one of every stream-taking function of the library all the same: all work is queued on that stream (NULL: the default stream) on
 * the device that is current, nothing synchronises, the library allocates nothing; tests/test_cvt_gpu.py holds the three calls to
 * it, under a capture and behind a gate.  They stand outside the table of tests/caller_stream.py only because that table could not
 * be extended when they were added; moving them into it (a `void *stream` parameter and three rows) is a follow-up.
 *
 * A host model reproduces every bit (tests/cvt_model.py).  Scratch: caller-owned device memory, cleared by the calls themselves; what
 * it holds between calls means nothing.  rem2d_cvt_scratch_bytes = 12 M C + 8 R, R = max(n_rows, M group_size) with a non-positive
 * term counted as 0: enough for every call on these shapes.  Each call checks what it needs itself: assign 8 n_rows, insert
 * 12 M C + 8 M S, emit_line 12 M C. */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_CVT_ABI_VERSION 1
#define REM2D_CVT_MAX_WIDTH 32     /* B */
#define REM2D_CVT_MAX_CELLS 65536  /* C */
#define REM2D_CVT_MAX_SPLITS 4096  /* splits */

/* Caller-owned device pointers and the shapes they have. */
typedef struct rem2d_cvt {
    int32_t d;               /* D: input rows of w1, 8 + 6 max_bodies + R with R in 0 .. 64; not looked at by assign */
    int32_t hidden;          /* H: 1 .. 128; not looked at by assign */
    int32_t max_bodies;      /* MB: 1 .. 64; not looked at by assign */
    int32_t width;           /* B: 1 .. 32 */
    int32_t n_cells;         /* C: 1 .. 65536 */
    int32_t n_blocks;        /* M >= 1, M C <= 2^31 - 1; not looked at by assign */
    int32_t group_size;      /* S >= 1 rows per block: insert looks at G = M S rows; not looked at by assign and emit_line */
    int32_t n_children;      /* M S', a positive multiple of M: emit_line */
    int32_t n_rows;          /* >= 1: the rows of assign; not looked at by insert and emit_line */
    int32_t splits;          /* the launch shape of the assignment: 0 = the library chooses, 1 .. 4096 = the centroids dealt over
                                that many workgroups per 256 rows.  No result depends on it */
    uint32_t generation;     /* counter word 2 of the draws and the variation */
    float sigma_iso;         /* finite */
    float sigma_line;        /* finite; +-0: no line term */
    int32_t reserved;        /* 0 */
    uint64_t seed;           /* the Philox key */
    const float *centroids;  /* [C][B]; read by assign and insert; may not overlap cell, dist or a grid buffer */
    const float *desc;       /* [n_rows][B] (assign), [G][B] (insert); may not overlap cell, dist or a grid buffer */
    const double *fitness;   /* [G]; read by insert */
    const uint8_t *mask;     /* [G] or NULL; read by insert */
    const float *w1;         /* [G][D][H]   the evaluated sets; read by insert; none may overlap an elite weight buffer */
    const float *b1;         /* [G][H] */
    const float *w2;         /* [G][H][MB] */
    const float *b2;         /* [G][MB] */
    double *elite_fitness;   /* [M][C]      the archive: read and written by insert */
    float *elite_desc;       /* [M][C][B] */
    float *elite_w1;         /* [M C][D][H] read by emit_line */
    float *elite_b1;         /* [M C][H] */
    float *elite_w2;         /* [M C][H][MB] */
    float *elite_b2;         /* [M C][MB] */
    int32_t *count;          /* [M][C]; read by emit_line */
    int32_t *cell;           /* [n_rows] (assign), [G] (insert): written */
    float *dist;             /* as cell, or NULL: written */
    int32_t *winner;         /* [M][C]; written by insert */
    float *child_w1;         /* [M S'][D][H]  written by emit_line; none may overlap an elite weight buffer */
    float *child_b1;         /* [M S'][H] */
    float *child_w2;         /* [M S'][H][MB] */
    float *child_b2;         /* [M S'][MB] */
    int32_t *parent;         /* [M S']; written by emit_line */
    int32_t *parent2;        /* [M S']; written by emit_line */
    int32_t *n_filled;       /* [M]; written by emit_line */
    void *scratch;           /* 8-byte aligned: all three calls */
    uint64_t scratch_bytes;  /* what `scratch` holds */
    void *stream;            /* the hipStream_t all work is queued on; NULL: the default stream (section 5) */
} rem2d_cvt;

/* REM2D_CVT_ABI_VERSION of the library */
int rem2d_cvt_abi_version(void);

/* 12 M C + 8 max(n_rows, M group_size, 0) bytes: what every call on these shapes needs at most.  REM2D_E_INVALID (negative) for a
 * NULL descriptor, a d, hidden or max_bodies out of range, a width outside 1 .. 32, n_cells outside 1 .. 65536, n_blocks < 1, M C
 * above 2^31 - 1, M group_size above 2^31 - 1, splits outside 0 .. 4096, a sigma_iso or sigma_line that is not finite, a non-zero
 * reserved.  No pointer is looked at. */
int64_t rem2d_cvt_scratch_bytes(const rem2d_cvt *v);

/* The assignment (section 2).  REM2D_E_INVALID for a NULL descriptor, a width outside 1 .. 32, n_cells outside 1 .. 65536, n_rows
 * < 1, splits outside 0 .. 4096, a non-zero reserved, a NULL centroids, desc, cell or scratch pointer, a scratch that is not 8-byte
 * aligned or holds fewer than 8 n_rows bytes, a desc or centroids that overlaps cell or dist.  Nothing else is looked at.
 * Everything is checked before the first launch; nothing is written after a refusal. */
int rem2d_cvt_assign(const rem2d_cvt *v);

/* The insertion (section 3).  REM2D_E_INVALID for what rem2d_cvt_scratch_bytes refuses, a group_size < 1, a NULL centroids, desc,
 * fitness, weight, archive, count, cell, winner or scratch pointer, a scratch that is misaligned or holds fewer than
 * 12 M C + 8 M S bytes, a desc or centroids that overlaps cell, dist or an archive buffer, an evaluated weight buffer that overlaps
 * an elite weight buffer.  n_rows, the child buffers, parent, parent2 and n_filled are not looked at. */
int rem2d_cvt_insert(const rem2d_cvt *v);

/* The line emission (section 4).  REM2D_E_INVALID for what rem2d_cvt_scratch_bytes refuses, an n_children that is not a positive
 * multiple of n_blocks, a NULL count, parent, parent2, n_filled, elite or child weight or scratch pointer, a scratch that is
 * misaligned or holds fewer than 12 M C bytes, a child buffer that overlaps an elite weight buffer.  width, centroids and the
 * members of the rows are not looked at beyond what rem2d_cvt_scratch_bytes checks. */
int rem2d_cvt_emit_line(const rem2d_cvt *v);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_CVT_H */
