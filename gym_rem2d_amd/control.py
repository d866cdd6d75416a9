"""Closed-loop control: the observation layout and the two library calls behind ``BatchedModular2D.observe`` /
``set_joint_targets`` / ``set_controllers`` (include/rem2d_control.h).

An observation row is float32 ``[OBS_HEAD + max_bodies * OBS_BODY]``: the root body's pose and velocity, its distance to the
wall of death and the body count, then six words per body in ``robot.components`` order.  ``layout(max_bodies)`` names the
columns.  A joint target is a write to two controller words between two steps (amp := 0, offset := target): the step kernels
compute ``(amp * sin(i_state + phase)) + offset`` as before and find ``offset``.
"""
import torch

from . import _lib

OBS_HEAD = 8          # REM2D_OBS_HEAD
OBS_BODY = 6          # REM2D_OBS_BODY
MAX_BODIES = 64       # REM2D_CONTROL_MAX_BODIES
CTRL_TARGET = 0       # REM2D_CTRL_TARGET
CTRL_PARAMS = 1       # REM2D_CTRL_PARAMS
ABI_VERSION = _lib.CONTROL_ABI_VERSION

HEAD_NAMES = ("root_px", "root_py", "root_ang", "root_vx", "root_vy", "root_w", "wod_distance", "n_bodies")
BODY_NAMES = ("joint_angle", "joint_speed", "limit_state", "touching", "dx", "dy")
# columns of a body's block
JOINT_ANGLE, JOINT_SPEED, LIMIT_STATE, TOUCHING, DX, DY = range(OBS_BODY)


def width(max_bodies):
    return OBS_HEAD + int(max_bodies) * OBS_BODY


class Layout:
    """Column names of an observation row.  ``head[name]`` is a column index, ``body[name]`` a slice over the bodies (column of
    body b: ``OBS_HEAD + b * OBS_BODY + k``), ``names`` the flat list; ``bodies(obs)`` views ``obs[..., OBS_HEAD:]`` as
    ``[..., max_bodies, OBS_BODY]``."""

    def __init__(self, max_bodies):
        self.max_bodies = int(max_bodies)
        self.width = width(max_bodies)
        self.head = {n: i for i, n in enumerate(HEAD_NAMES)}
        self.body = {n: slice(OBS_HEAD + k, self.width, OBS_BODY) for k, n in enumerate(BODY_NAMES)}
        self.names = list(HEAD_NAMES) + ["body%d_%s" % (b, n) for b in range(self.max_bodies) for n in BODY_NAMES]

    def bodies(self, obs):
        return obs[..., OBS_HEAD:].reshape(obs.shape[:-1] + (self.max_bodies, OBS_BODY))


def layout(max_bodies):
    return Layout(max_bodies)


def _check_bodies(max_bodies):
    if not 1 <= int(max_bodies) <= MAX_BODIES:
        raise ValueError("max_bodies must be 1..%d, not %r" % (MAX_BODIES, max_bodies))


def observe(worlds, max_bodies, out):
    """rem2d_worlds_observe for a list of BatchedWorld (one build, one device) on the current stream.  ``out``: contiguous
    float32 ``[rows, width(max_bodies)]`` on the worlds' device."""
    _check_bodies(max_bodies)
    w0 = worlds[0]
    if out.dtype != torch.float32 or not out.is_contiguous() or out.device != w0.device or out.dim() != 2 \
            or out.shape[1] != width(max_bodies):
        raise ValueError("observe: out must be a contiguous float32 [rows, %d] tensor on %s" % (width(max_bodies), w0.device))
    _lib.check(w0.L.rem2d_worlds_observe(_lib.world_array(worlds), len(worlds), int(max_bodies), out.data_ptr(), out.shape[0],
                                         w0._stream()), w0.wide)
    return out


def control(worlds, mode, values, mask=None):
    """rem2d_worlds_control for a list of BatchedWorld on the current stream.  ``values``: ``[rows, max_bodies]`` (CTRL_TARGET)
    or ``[rows, max_bodies, 4]`` (CTRL_PARAMS: amp, phase, freq, offset), any float dtype, any device; ``mask``: optional
    ``[rows, max_bodies]``, false = leave the joint as it is.  Asynchronous for tensors that are on the worlds' device already (a
    dtype conversion is one more kernel on the same stream); a host array or a tensor of another device is uploaded first, which
    blocks the host until the copy is done.  Returns the device tensors the queued kernel reads (the caller keeps them until the
    next call: nothing here waits for the kernel)."""
    w0 = worlds[0]
    values = torch.as_tensor(values)
    want = 2 if mode == CTRL_TARGET else 3
    if values.dim() != want or (mode == CTRL_PARAMS and values.shape[2] != 4):
        raise ValueError("control: values must be [rows, max_bodies]%s" % ("" if mode == CTRL_TARGET else " x 4"))
    _check_bodies(values.shape[1])
    values = values.to(device=w0.device, dtype=torch.float64).contiguous()   # (float32 -> float64 is exact)
    mask_ptr = None
    if mask is not None:
        mask = torch.as_tensor(mask)
        if tuple(mask.shape) != tuple(values.shape[:2]):
            raise ValueError("control: mask must be [rows, max_bodies] like the values")
        mask = (mask != 0).to(device=w0.device, dtype=torch.uint8).contiguous()
        mask_ptr = mask.data_ptr()
    _lib.check(w0.L.rem2d_worlds_control(_lib.world_array(worlds), len(worlds), int(mode), values.data_ptr(), int(values.shape[1]),
                                         int(values.shape[0]), mask_ptr, w0._stream()), w0.wide)
    return values, mask
