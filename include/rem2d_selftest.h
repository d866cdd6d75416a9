#ifndef REM2D_SELFTEST_H
#define REM2D_SELFTEST_H

/* Self-test of the collision geometry of librem2d.so: the device's narrowphase routines, b2Distance, b2TimeOfImpact and the
 * exact skip in front of it, run on a table of cases that the CALLER chose -- one lane per case -- and written out word for
 * word.  The step kernels reach these routines only with the pairs of shapes their dynamics produce; a test reaches them here
 * with the inputs on which such routines go wrong (a separation exactly at a radius, a tie between two faces, a vertex on a
 * line), and compares every word with its own reference (tests/test_geometry_gpu.py: the CPU oracle's known-answer entry
 * points).  Kept in a header of its own: nothing here changes what a step computes, and include/rem2d.h stays as it is.
 *
 * A lane builds its arguments exactly as the step kernels do: the static shape A at the identity (an isolated edge, or a
 * hardcore box as the four vertices and four normals rem2d_world_set_terrain derives -- rem2d_selftest_static_box is that host
 * code), the module shape B (a SetAsBox box of half-extents hx, hy, or a circle of radius hx) at a pose, and calls the same
 * device functions the step kernels call.
 *
 * A case is REM2D_SELFTEST_CASE_WORDS binary32 words (case_words >= that; the rest of a row is ignored):
 *    0      kind of A: 0 = edge, 1 = static box
 *    1- 8   A's vertices x0 y0 .. x3 y3 (an edge uses the first two)
 *    9-16   A's normals  x0 y0 .. x3 y3 (static box only)
 *   17      shape of B: 1 = box, 2 = circle
 *   18-19   hx, hy (circle: radius, unused)
 *   20-22   c0.x c0.y a0: B's pose (COLLIDE, DISTANCE), the start of its sweep (TOI, FAR_APART)
 *   23-25   c.x  c.y  a : the end of its sweep (TOI, FAR_APART)
 * Every case writes REM2D_SELFTEST_OUT_WORDS words to fout_dev [n][8] and to iout_dev [n][8]; words an op does not use are 0:
 *   COLLIDE    iout: manifold type, point count, feature key 0, key 1      fout: localNormal.xy localPoint.xy p0.xy p1.xy
 *   DISTANCE   iout: simplex count, indexA[3], indexB[3] (-1 past count)    fout: distance of the core shapes, cache metric
 *              (b2Distance from an empty cache, useRadii = false)
 *   TOI        iout: state (0 unknown 1 failed 2 overlapped 3 touching 4 separated)       fout: t     (tMax = 1, A static)
 *   FAR_APART  iout: 1 where the step kernels skip b2TimeOfImpact for this pair and take alpha = 1, else 0 */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_SELFTEST_ABI_VERSION 1
#define REM2D_SELFTEST_CASE_WORDS 26
#define REM2D_SELFTEST_OUT_WORDS 8

enum { REM2D_SELFTEST_COLLIDE = 0, REM2D_SELFTEST_DISTANCE = 1, REM2D_SELFTEST_TOI = 2, REM2D_SELFTEST_FAR_APART = 3,
       REM2D_SELFTEST_OP_COUNT = 4 };

/* REM2D_SELFTEST_ABI_VERSION of the library */
int rem2d_selftest_abi_version(void);

/* Host only: a hardcore box as rem2d_world_set_terrain stores it.  xy: the four corners [4][2] as the terrain lists them;
 * out16: vertices x0 y0 .. x3 y3 in hull order, then the four edge normals (words 1-16 of a case).  REM2D_E_INVALID for NULL
 * arguments and for corners that are no convex quad. */
int rem2d_selftest_static_box(const float *xy, float *out16);

/* Runs `op` on cases_dev [n][case_words], one lane per case.  Device pointers; asynchronous on `stream`; allocates nothing.
 * n = 0 is a no-op.  REM2D_E_INVALID, before anything is dereferenced or launched, for an unknown op, n < 0,
 * case_words < REM2D_SELFTEST_CASE_WORDS and a NULL pointer with n > 0.  A case whose kind or shape word is none of the values
 * above writes -1 to iout[0] and 0 to its other words. */
int rem2d_selftest_geometry(int32_t op, int32_t n, const float *cases_dev, int32_t case_words, float *fout_dev, int32_t *iout_dev,
                            int32_t device, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_SELFTEST_H */
