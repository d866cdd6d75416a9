#ifndef REM2D_CONTROL_H
#define REM2D_CONTROL_H

/* Closed-loop control for librem2d.so: what a population senses, as float32 rows in population order, and what a caller
 * sets on its joints between two steps, both on the device and both for a WHOLE population (all lane buckets, all step
 * groups) in one launch.  Kept apart from include/rem2d.h: that header is the physics ABI the CPU twin (oracle/rem2d_cpu.c)
 * restates entry for entry, and nothing here changes what a step computes.
 *
 * The reference fills neither side: Modular2D.step(action) ignores `action` and returns observation = 0
 * (Modular2DEnv.py:607-653); every joint follows its node's open-loop oscillator (Controller/m_controller.py:17-21).
 *
 * How a joint target reaches the motor without touching a step kernel: a step computes, in binary64,
 *     target     = (amp * sin(i_state + phase)) + offset
 *     motorSpeed = (float)((target - (double)jointAngle) * 1.9)
 * With amp == 0.0 the product is +-0 for every finite argument of the sine, so target == offset exactly: a closed-loop joint
 * target is a write to two controller words of the state arena (REM2D_F_CAMP := 0, REM2D_F_COFFSET := target) between two
 * steps.  i_state keeps integrating (+= freq per step) and is never written here. */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_CONTROL_ABI_VERSION 1
#define REM2D_CONTROL_MAX_BODIES 64 /* largest max_bodies (= REM2D_MAX_LANES) */

/* An observation row: REM2D_OBS_HEAD + max_bodies * REM2D_OBS_BODY float32 words.
 *   head  0..5  the root body's px, py, ang, vx, vy, w
 *         6     (float)((double)px_root - wall_of_death): the distance to the wall of death
 *         7     number of bodies
 *   body b (b < max_bodies), at REM2D_OBS_HEAD + b * REM2D_OBS_BODY:
 *         0     joint angle to the parent body, ang - ang_parent - 0.0f: the expression a step feeds the PID
 *         1     joint speed, w - w_parent (b2RevoluteJoint::GetJointSpeed)
 *         2     the joint's limit state (REM2D_F_JLIMIT: 0 inactive, 1 at lower, 2 at upper, 3 equal)
 *         3     touching contacts: the body's pair slots whose manifold has at least one point
 *         4, 5  px - px_root, py - py_root
 * Body b is the b-th live lane (shape != 0) of the creature, in lane order: the order of robot.components.  Body 0 is the
 * root: its words 0..2 and 4..5 are 0.  Body slots beyond the creature's count are 0, bodies beyond max_bodies are dropped.
 * Every word is a copy, an exact int -> float conversion or ONE separately rounded binary32 operation, so the
 * -ffp-contract=fast build writes the same bits as the default one.  (Room for range sensing is left behind the body
 * block: a later version appends, it does not move these words.  The ray fractions themselves come from a call of their own,
 * include/rem2d_sense.h, as rows of their own in the same population order; the gym facade puts them behind these words.) */
#define REM2D_OBS_HEAD 8
#define REM2D_OBS_BODY 6

/* rem2d_worlds_control modes */
#define REM2D_CTRL_TARGET 0 /* values [n_rows][max_bodies]:    amp := 0.0, offset := v */
#define REM2D_CTRL_PARAMS 1 /* values [n_rows][max_bodies][4]: amp, phase, freq, offset := v[0..3] */

/* REM2D_CONTROL_ABI_VERSION of the library */
int rem2d_control_abi_version(void);

/* Observation rows of every creature of `worlds` (any number: all lane buckets and step groups of a population; one launch
 * per 16 worlds) into out_dev: float32 [out_rows][REM2D_OBS_HEAD + max_bodies * REM2D_OBS_BODY].  Creature e of a world goes
 * to row index[e], `index` being the population index rem2d_world_set_outputs installed, or to row e without one; a row
 * outside [0, out_rows) is skipped.  max_bodies: 1 .. REM2D_CONTROL_MAX_BODIES.  The worlds must share a device and have been
 * reset (or adopted).  Device pointers; asynchronous on `stream`; nothing is allocated or loaded on a first call.
 * REM2D_E_INVALID for a NULL pointer, n_worlds <= 0, max_bodies or out_rows out of range or a world of more than 64 lanes
 * per creature; REM2D_E_STATE before rem2d_world_reset. */
int rem2d_worlds_observe(rem2d_world *const *worlds, int32_t n_worlds, int32_t max_bodies, float *out_dev, int64_t out_rows,
                         void *stream);

/* Writes the controller words of the jointed live bodies of every creature of `worlds` from values_dev (binary64, rows in
 * the population order of rem2d_worlds_observe): column b drives the joint between body b and its parent, column 0 (the
 * root has no joint) is ignored, joints of bodies beyond max_bodies and creatures whose row is outside [0, n_rows) are left
 * as they are.  mode: REM2D_CTRL_TARGET or REM2D_CTRL_PARAMS.  mask_dev: NULL, or uint8 [n_rows][max_bodies] where 0 means
 * "leave this joint as it is".  REM2D_F_CISTATE is never written.  The values are written AS GIVEN, non-finite ones
 * included: a step clamps nothing between the controller and the motor speed either, so keeping a target inside the joint's
 * limits (and finite) is the caller's business.  Takes effect with the next step queued on the same stream.  Arguments and
 * errors as rem2d_worlds_observe. */
int rem2d_worlds_control(rem2d_world *const *worlds, int32_t n_worlds, int32_t mode, const double *values_dev,
                         int32_t max_bodies, int64_t n_rows, const uint8_t *mask_dev, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_CONTROL_H */
