#ifndef REM2D_SENSE_H
#define REM2D_SENSE_H

/* Terrain range sensing for librem2d.so: what BipedalWalker calls lidar.  For every creature of a population and every ray of a
 * caller's table, the fraction of the ray at which it first meets the track (its edges and, on the hardcore track, its boxes),
 * computed on the device for a WHOLE population (all lane buckets, all step groups) in one launch.  The companion of
 * include/rem2d_control.h, kept in a header of its own: that one is pinned to its three functions, and nothing here changes
 * what a step or an observation row holds.
 *
 * The reference inherits the pieces from BipedalWalker and fills none of them: observation_space is Box(-inf, inf, (24,)) = 14
 * proprioceptive values + 10 lidar fractions, LIDAR_RANGE = 160 / SCALE (Modular2DEnv.py:32), and a `lidar` list that render
 * would draw (:741-744) stays empty.
 *
 * A ray: p1 = the root body's (px, py), binary32; p2 = ((float)((double)px + off.x), (float)((double)py + off.y)) with the
 * caller's binary64 offset -- the position widened, added to in binary64 and narrowed once, as pybox2d does with Python
 * arithmetic on a body.position; d = p2 - p1 in binary32; maxFraction = 1.  Every static proxy of the world's terrain is a
 * candidate: b2EdgeShape::RayCast for the isolated edges (two-sided), b2PolygonShape::RayCast for the boxes (a ray that starts
 * inside a box does not hit it).  Rays are fixed in the world frame: they do not turn with the root.
 *
 * The result is the smallest fraction over all proxies, 1.0f where there is none, and the index of that proxy: boxes are
 * 0 .. n_polys-1, edge i (xs[i] -> xs[i + 1]) is n_polys + i -- the order of rem2d_world_set_terrain, which is creation order --
 * and -1 means no hit.  Among equal fractions the lowest index wins (a ray through a vertex shared by two edges reports the
 * first of them).  A creature whose root position is not finite reads 1.0f / -1.  Every arithmetic result is one separately
 * rounded binary32 operation in every build of the library: the -ffp-contract=fast build writes the same bits. */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_SENSE_ABI_VERSION 1
#define REM2D_SENSE_MAX_RAYS 64

/* REM2D_SENSE_ABI_VERSION of the library */
int rem2d_sense_abi_version(void);

/* Ray fractions of every creature of `worlds` (any number: all lane buckets and step groups of a population; one launch per 16
 * worlds) into frac_dev: float32 [rows][n_rays], and, unless hit_dev is NULL, the proxy indices into hit_dev: int32
 * [rows][n_rays].  ray_offsets_dev: binary64 [n_rays][2] = (x, y) of p2 - p1, n_rays: 1 .. REM2D_SENSE_MAX_RAYS.  Creature e of
 * a world goes to row index[e], `index` being the population index rem2d_world_set_outputs installed, or to row e without one; a
 * row outside [0, rows) is skipped.  Every world is cast against its own terrain.  Device pointers; asynchronous on `stream`;
 * nothing is allocated or loaded on a first call.
 * REM2D_E_INVALID for no worlds, a NULL ray_offsets_dev or frac_dev, n_rays or rows out of range, a NULL world, worlds of
 * different devices or of more than 64 lanes per creature; REM2D_E_STATE before rem2d_world_set_terrain or before
 * rem2d_world_reset (or adopt). */
int rem2d_worlds_sense(rem2d_world *const *worlds, int32_t n_worlds, const double *ray_offsets_dev, int32_t n_rays, float *frac_dev,
                       int32_t *hit_dev, int64_t rows, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_SENSE_H */
