#ifndef REM2D_RENDER_H
#define REM2D_RENDER_H

/* The creature renderer of librem2d.so: RGB frames of creatures drawn straight from a world's state arena and uploaded terrain, on
 * the device.  Kept apart from include/rem2d.h: that header is the physics ABI the CPU twin (oracle/rem2d_cpu.c) restates entry for
 * entry; a picture is nothing the physics computes.
 *
 * The scene is the one gym_rem2D's Modular2DEnv.render draws (Modular2DEnv.py:655-738): sky, ground, terrain edges, hardcore
 * obstacles, the creature's bodies in slot order, the wall of death and the flag, at SCALE = 30 pixels per metre.  Every pixel is
 * defined exactly (binary32, + - * and comparisons only: gym_rem2d_amd/csrc/rem2d_raster.h), so that a CPU model reproduces it
 * bit for bit. */

#include "rem2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_RENDER_ABI_VERSION 1
#define REM2D_RENDER_MAX_SIZE 8192 /* largest width / height */

/* Draws n creatures of the world `w` into out_dev: uint8 [n][height][width][3] (HWC RGB, gym's rgb_array layout).
 *   creatures_dev  int32 [n]: the world's creature index (0 .. n_envs - 1) of each image; read back to the host and checked
 *                  (a synchronising copy on `stream`)
 *   cam_xy_dev     float [n][2]: the world coordinates of the view's lower left corner (the reference's scroll, scroll_y);
 *                  pixel (i, j) has its centre at (cam_x + (i + 0.5) / 30, cam_y + height / 30 - (j + 0.5) / 30)
 *   fill_rgb_dev,  uint8 [n_envs][lanes][3]: fill / outline colour of every body of the world, or NULL for a fixed colour
 *   line_rgb_dev   pair per shape
 * Device pointers; asynchronous on `stream` after the index check.  REM2D_E_INVALID for a NULL pointer, n < 0, a size outside
 * 1 .. REM2D_RENDER_MAX_SIZE or a creature index outside the world; REM2D_E_STATE before rem2d_world_set_terrain. */
int rem2d_world_render(const rem2d_world *w, const int32_t *creatures_dev, int32_t n, const float *cam_xy_dev,
                       const uint8_t *fill_rgb_dev, const uint8_t *line_rgb_dev, int32_t width, int32_t height, uint8_t *out_dev,
                       void *stream);

/* REM2D_RENDER_ABI_VERSION of the library */
int rem2d_render_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_RENDER_H */
