#ifndef REM2D_POLICY_H
#define REM2D_POLICY_H

/* Device policies for librem2d.so: a small feed-forward controller per creature (or one shared by many), evaluated for a WHOLE
 * population by one kernel between what the creatures sense (include/rem2d_control.h rem2d_worlds_observe, include/rem2d_sense.h
 * rem2d_worlds_sense) and what their joints are told (rem2d_worlds_control).  A header of its own, like those two: nothing here
 * changes what a step, an observation row or a ray fraction holds.
 *
 * The policy is data: weights in device memory, owned by the caller.  For population row r, with MB = max_bodies and R rays:
 *
 *   input    x    = the D = 8 + 6 MB + R binary32 words of row r: the observation row, then the R ray fractions
 *   weights  g    = index[r], or r without an index; set g holds w1[D][H], b1[H], w2[H][MB], b2[MB] (binary32, contiguous,
 *                   input index major; the sets follow each other in each of the four arrays)
 *   hidden   a_j  = b1[j];  for i = 0 .. D-1 in ascending order:  a_j = a_j + (x_i * w1[i][j])
 *            h_j  = a_j / (1.0f + |a_j|)       (REM2D_POLICY_SOFTSIGN)
 *                 = a_j > 0 ? a_j : 0.0f       (REM2D_POLICY_RELU: NaN and -0 give +0)
 *   output   y_m  = b2[m];  for j = 0 .. H-1 in ascending order:  y_m = y_m + (h_j * w2[j][m])
 *   target   t_m  = scale * (y_m / (1.0f + |y_m|)),   targets[r][m] = (double)t_m,   valid[r][m] = isfinite(t_m)
 *
 * Every product, sum and quotient is one separately, correctly rounded binary32 operation -- nothing is fused, in any build of
 * the library (the -ffp-contract=fast build writes the same bits) -- and there is no transcendental function: a host model in
 * binary32 reproduces every bit (tests/policy_model.py).  A target that is not finite never reaches a joint: `valid` is the mask
 * rem2d_worlds_act hands to rem2d_worlds_control.  The library allocates nothing. */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_POLICY_ABI_VERSION 1
#define REM2D_POLICY_MAX_HIDDEN 128
#define REM2D_POLICY_SOFTSIGN 0
#define REM2D_POLICY_RELU 1

/* Caller-owned device pointers and the shapes they have. */
typedef struct rem2d_policy {
    int32_t d;             /* words of an input row: must be 8 + 6 * max_bodies + n_rays */
    int32_t max_bodies;    /* MB: 1 .. 64 (REM2D_CONTROL_MAX_BODIES) */
    int32_t n_rays;        /* R: 0 .. 64 (REM2D_SENSE_MAX_RAYS) */
    int32_t hidden;        /* H: 1 .. REM2D_POLICY_MAX_HIDDEN */
    int32_t activation;    /* REM2D_POLICY_SOFTSIGN | REM2D_POLICY_RELU */
    float scale;           /* the joint target is scale * softsign(y); (float)(pi / 2) is the reference's joint limit */
    int32_t n_sets;        /* G >= 1 weight sets */
    int32_t reserved;      /* 0 */
    const float *w1;       /* [G][D][H] */
    const float *b1;       /* [G][H] */
    const float *w2;       /* [G][H][MB] */
    const float *b2;       /* [G][MB] */
    const int32_t *index;  /* [n_rows] weight set of a row, or NULL: row r uses set r (then G must be n_rows).  A value outside
                              [0, G) skips the row */
    const uint8_t *row_mask; /* [n_rows] or NULL: 0 skips the row.  A skipped row's outputs stay untouched */
    const float *obs;      /* [n_rows][8 + 6 MB]: what rem2d_worlds_observe wrote (max_bodies = MB) */
    const float *frac;     /* [n_rows][R]: what rem2d_worlds_sense wrote; may be NULL when R == 0 */
    double *targets;       /* [n_rows][MB], written */
    uint8_t *valid;        /* [n_rows][MB], written */
    int64_t n_rows;        /* N >= 0 population rows */
} rem2d_policy;

/* REM2D_POLICY_ABI_VERSION of the library */
int rem2d_policy_abi_version(void);

/* The forward pass alone, on whatever the rows of p->obs / p->frac hold: one kernel on `stream`, asynchronous, on the device that
 * is current.  REM2D_E_INVALID for a NULL p or a NULL array (index, row_mask and, with n_rays == 0, frac may be NULL), a
 * dimension out of range, d != 8 + 6 max_bodies + n_rays, an unknown activation, n_sets < 1, n_rows < 0, and n_sets != n_rows
 * without an index. */
int rem2d_policy_forward(const rem2d_policy *p, void *stream);

/* One control step of a population: rem2d_worlds_observe (max_bodies = p->max_bodies) into p->obs, rem2d_worlds_sense with
 * ray_offsets_dev (binary64 [n_rays][2]) into p->frac if n_rays > 0, the forward pass, and rem2d_worlds_control in
 * REM2D_CTRL_TARGET mode with p->targets as the values and p->valid as the mask: four launches (per 16 worlds) queued on `stream`
 * by one call, asynchronous.  Rows are population rows as rem2d_world_set_outputs' index names them.  Everything is checked before
 * the first launch: what rem2d_policy_forward refuses, no worlds, a NULL ray_offsets_dev with n_rays > 0, and what the three calls
 * refuse for their worlds (REM2D_E_STATE before rem2d_world_reset, and with n_rays > 0 before rem2d_world_set_terrain). */
int rem2d_worlds_act(rem2d_world *const *worlds, int32_t n_worlds, const rem2d_policy *p, const double *ray_offsets_dev, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_POLICY_H */
