"""Terrain range sensing: the ray tables and the library call behind ``BatchedModular2D.sense_terrain``
(include/rem2d_sense.h).

A ray is a binary64 offset from a creature's root body; its result is the fraction of the ray at which it first meets the track
(1.0: nothing within reach) and, on request, the index of the static proxy it met (hardcore boxes ``0 .. n_polys - 1``, then edge
``i`` as ``n_polys + i``; ``-1``: none).  ``bipedal_rays()`` is BipedalWalker's lidar fan, whose 10 fractions are the part of the
reference's advertised 24-float observation that the reference itself never fills (Modular2DEnv.py:32, :741-744).
"""
import math

import numpy as np
import torch

from . import _lib

LIDAR_RANGE = 160 / 30.0      # Modular2DEnv.py:32: 160 / SCALE
MAX_RAYS = _lib.SENSE_MAX_RAYS
ABI_VERSION = _lib.SENSE_ABI_VERSION
NO_HIT = -1


def bipedal_rays(n=10):
    """BipedalWalker's lidar fan as offsets float64 ``[n, 2]``: ray i reaches ``(sin(1.5 i / n), -cos(1.5 i / n)) * LIDAR_RANGE``
    from the root, from straight down (i = 0) to about 77 degrees forward.  Recalled from gym's BipedalWalker (its step() casts
    ``lidar[i].p2 = (pos[0] + sin(1.5 * i / 10) * LIDAR_RANGE, pos[1] - cos(1.5 * i / 10) * LIDAR_RANGE)``); gym is not a
    dependency here and the fan is pinned to no recording."""
    return np.array([(math.sin(1.5 * i / n) * LIDAR_RANGE, -math.cos(1.5 * i / n) * LIDAR_RANGE) for i in range(n)],
                    dtype=np.float64).reshape(n, 2)


def check_rays(rays):
    """The ray table as a contiguous float64 ``[R, 2]`` numpy array, R in 1 .. MAX_RAYS."""
    rays = np.ascontiguousarray(np.asarray(rays, dtype=np.float64))
    if rays.ndim != 2 or rays.shape[1] != 2 or not 1 <= rays.shape[0] <= MAX_RAYS:
        raise ValueError("rays must be [R, 2] offsets with R in 1..%d, not %r" % (MAX_RAYS, rays.shape))
    return rays


def sense(worlds, rays, frac, hit=None):
    """rem2d_worlds_sense for a list of BatchedWorld (one build, one device) on the current stream.  ``rays``: contiguous float64
    ``[R, 2]`` on the worlds' device; ``frac``: contiguous float32 ``[rows, R]``; ``hit``: None or contiguous int32 ``[rows, R]``."""
    w0 = worlds[0]
    if rays.dtype != torch.float64 or not rays.is_contiguous() or rays.device != w0.device or rays.dim() != 2 or rays.shape[1] != 2 \
            or not 1 <= rays.shape[0] <= MAX_RAYS:
        raise ValueError("sense: rays must be a contiguous float64 [R, 2] tensor on %s, R in 1..%d" % (w0.device, MAX_RAYS))
    R = int(rays.shape[0])
    if frac.dtype != torch.float32 or not frac.is_contiguous() or frac.device != w0.device or frac.dim() != 2 or frac.shape[1] != R:
        raise ValueError("sense: frac must be a contiguous float32 [rows, %d] tensor on %s" % (R, w0.device))
    if hit is not None and (hit.dtype != torch.int32 or not hit.is_contiguous() or hit.device != w0.device
                            or tuple(hit.shape) != tuple(frac.shape)):
        raise ValueError("sense: hit must be a contiguous int32 tensor of frac's shape on %s" % w0.device)
    _lib.check(w0.L.rem2d_worlds_sense(_lib.world_array(worlds), len(worlds), rays.data_ptr(), R, frac.data_ptr(),
                                       None if hit is None else hit.data_ptr(), int(frac.shape[0]), w0._stream()), w0.wide)
    return frac if hit is None else (frac, hit)
