"""Frames of creatures, drawn on the GPU from the state the stepper already holds (include/rem2d_render.h).

The scene is the one ``Modular2DEnv.render`` draws (``gym_rem2D/envs/Modular2DEnv.py:655-738``): sky, ground, terrain edges,
hardcore obstacles, the creature's bodies, the wall of death and the flag, at SCALE = 30 pixels per metre, as uint8
``[n, H, W, 3]`` (gym's ``rgb_array`` layout, one image per creature).  ``render_frames`` draws creatures of a
:class:`~gym_rem2d_amd.env.BatchedModular2D` as they stand; ``record_frames`` steps one through an episode and hands its frames
to the host in bounded chunks; ``write_png`` / ``write_npy`` put them on disk.  Every pixel is defined exactly (binary32,
``csrc/rem2d_raster.h``), so a CPU model can reproduce a frame bit for bit.
"""
import os

import numpy as np
import torch

from . import _lib

SCALE = 30.0
VIEWPORT_W, VIEWPORT_H = 800, 600

# the palette: round(255 * c) of the reference's colours (csrc/rem2d_raster.h RC_*)
SKY = (230, 230, 255)
GROUND = (102, 153, 76)
EDGE_EVEN, EDGE_ODD = (76, 255, 76), (76, 204, 76)
OBSTACLE_FILL, OBSTACLE_LINE = (255, 255, 255), (153, 153, 153)
WALL_OF_DEATH = (0, 0, 255)
FLAG_LINE, FLAG_FILL = (0, 0, 0), (230, 51, 0)
# bodies without a colour of their own (array populations, or rem2d_world_render's NULL tables): one pair per shape
BOX_FILL, BOX_LINE = (127, 166, 217), (31, 63, 102)
CIRCLE_FILL, CIRCLE_LINE = (217, 166, 127), (102, 64, 31)

SHAPE_BOX, SHAPE_CIRCLE = 1, 2


def to_uint8(rgb):
    """round(255 * c) per channel (Python's round, as the palette)."""
    return tuple(int(round(255 * float(c))) for c in rgb[:3])


def _viridis():
    import matplotlib
    return matplotlib.colormaps["viridis"]


def tree_colors(tree, module_list, lanes):
    """(fill, line) uint8 [lanes, 3] of one creature built from ``tree``: the reference's rule, ``color1 = color2 =
    viridis(node.type / len(module_list))`` (simple_module.py:299-304, circular_module.py:204-211); bodies of nodes without a
    module list get the fixed colour of their shape."""
    fill = np.zeros((lanes, 3), np.uint8)
    line = np.zeros((lanes, 3), np.uint8)
    cmap = _viridis() if module_list else None
    for node in tree.getNodes() if hasattr(tree, "getNodes") else tree.nodes:
        comp = getattr(node, "component", None)
        if not (getattr(node, "expressed", False) and comp):
            continue
        body = comp[0]
        if cmap is not None:
            c = to_uint8(cmap(node.type / len(module_list)))
            fill[body.slot] = line[body.slot] = c
        else:
            circle = body.shape == SHAPE_CIRCLE
            fill[body.slot] = CIRCLE_FILL if circle else BOX_FILL
            line[body.slot] = CIRCLE_LINE if circle else BOX_LINE
    return fill, line


def _locate(env, creatures):
    """population index -> (world index, the creature's index in that world), the mapping _gather uses: every world that is
    still stepped lists the population indices of its creatures (compact() replaces and retires worlds)."""
    n = env.n_envs
    where = np.full(n, -1, np.int64)
    local = np.full(n, -1, np.int64)
    for wi, (w, idx) in enumerate(env.worlds):
        if wi in getattr(env, "_inactive", ()) or getattr(w, "h", None) is None:
            continue
        pop = idx.cpu().numpy()
        where[pop] = wi
        local[pop] = np.arange(len(pop))
    req = np.asarray(list(creatures), dtype=np.int64).reshape(-1)
    bad = (req < 0) | (req >= n)
    if bad.any():
        raise IndexError("creature %d is outside the population of %d" % (int(req[bad][0]), n))
    gone = where[req] < 0
    if gone.any():
        raise ValueError("creature %d is no longer stepped (compact() dropped it: its fitness was final)" % int(req[gone][0]))
    return req, where[req], local[req]


def _world_colors(env, wi):
    """(fill, line) device uint8 [n_envs][lanes][3] of world wi from the env's trees, or (None, None): the shape colours.
    Cached per world object (compact() makes new ones)."""
    if env.trees is None or len(env.trees) != env.n_envs:
        return None, None
    cache = env.__dict__.setdefault("_render_colors", {})
    w, idx = env.worlds[wi]
    hit = cache.get(wi)
    if hit is not None and hit[0] is w:
        return hit[1], hit[2]
    lists = getattr(env, "module_lists", None) or [None] * env.n_envs
    fill = np.zeros((w.n_envs, w.lanes, 3), np.uint8)
    line = np.zeros_like(fill)
    for e, p in enumerate(idx.cpu().tolist()):
        fill[e], line[e] = tree_colors(env.trees[p], lists[p], w.lanes)
    f, l_ = (torch.from_numpy(a).to(w.device) for a in (fill, line))
    cache[wi] = (w, f, l_)
    return f, l_


def root_poses(env, creatures):
    """float64 [n, 2]: (x, y) of the root body (slot 0) of each creature, on the device."""
    req, wis, loc = _locate(env, creatures)
    out = torch.empty((len(req), 2), dtype=torch.float64, device=env.worlds[0][0].device)
    for wi in np.unique(wis):
        pos = np.nonzero(wis == wi)[0]
        w = env.worlds[wi][0]
        li = torch.as_tensor(loc[pos], device=w.device)
        at = torch.as_tensor(pos, device=w.device)
        out[at, 0] = w.view("px")[li, 0].double()
        out[at, 1] = w.view("py")[li, 0].double()
    return out


class ReferenceCamera:
    """The reference's stateful scroll (Modular2DEnv.py:636-641) for n creatures, kept as float64 device tensors: after every
    step ``x_scroll = root_x - VIEWPORT_W / SCALE / 5``, ``scroll = x_scroll + 0.99 (x_scroll - prevscroll)``, ``prevscroll =
    x_scroll`` (the same in y with VIEWPORT_H / SCALE / 4); reset() starts everything at 0 (:575-579).  ``xy`` is the
    [n, 2] float32 view corner rem2d_world_render takes."""

    def __init__(self, n, device=None):
        z = torch.zeros(n, dtype=torch.float64, device=device)
        self.scroll, self.scroll_y, self.prevscroll, self.prevscroll_y = z.clone(), z.clone(), z.clone(), z.clone()

    def update(self, root_x, root_y):
        """One env step: the root's position after it (float64 tensors [n] or what torch.as_tensor takes)."""
        dev = self.scroll.device
        x_scroll = torch.as_tensor(root_x, dtype=torch.float64, device=dev) - VIEWPORT_W / SCALE / 5
        y_scroll = torch.as_tensor(root_y, dtype=torch.float64, device=dev) - VIEWPORT_H / SCALE / 4
        self.scroll = x_scroll + 0.99 * (x_scroll - self.prevscroll)
        self.scroll_y = y_scroll + 0.99 * (y_scroll - self.prevscroll_y)
        self.prevscroll, self.prevscroll_y = x_scroll, y_scroll
        return self

    @property
    def xy(self):
        return torch.stack([self.scroll, self.scroll_y], dim=1).float().contiguous()


def reference_camera(n=1, device=None):
    """A :class:`ReferenceCamera` in its reset() state."""
    return ReferenceCamera(n, device)


def follow_camera(env, creatures):
    """float32 [n, 2]: a view that puts each root where the reference's scroll settles (1/5 from the left, 1/4 from the bottom of
    the 800 x 600 view) -- for a single frame, which has no previous step to smooth with."""
    p = root_poses(env, creatures)
    return torch.stack([p[:, 0] - VIEWPORT_W / SCALE / 5, p[:, 1] - VIEWPORT_H / SCALE / 4], dim=1).float().contiguous()


def render_frames(env, creatures, width=VIEWPORT_W, height=VIEWPORT_H, camera=None, fill=None, line=None, out=None):
    """uint8 [n, height, width, 3] on the device: the creatures (population indices of ``env``) as they stand now.  camera: a
    :class:`ReferenceCamera`, float [n, 2] view corners (world coordinates of the lower left corner), or None for
    :func:`follow_camera`.  fill / line: uint8 [n_envs, lanes, 3] tables for a single-world env, or None for the env's own
    colours (the trees' viridis colours when it was reset from trees, otherwise one colour per shape).  One launch per world
    that holds requested creatures, on the current stream."""
    width, height = int(width), int(height)
    if not (1 <= width <= _lib.RENDER_MAX_SIZE and 1 <= height <= _lib.RENDER_MAX_SIZE):
        raise ValueError("image size %d x %d: width and height must be 1..%d" % (width, height, _lib.RENDER_MAX_SIZE))
    req, wis, loc = _locate(env, creatures)
    dev = env.worlds[0][0].device
    n = len(req)
    if camera is None:
        cam = follow_camera(env, req)
    elif isinstance(camera, ReferenceCamera):
        cam = camera.xy
    else:
        cam = torch.as_tensor(camera, dtype=torch.float32, device=dev).reshape(n, 2).contiguous()
    if cam.shape[0] != n:
        raise ValueError("camera holds %d views for %d creatures" % (cam.shape[0], n))
    if out is None:
        out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != (n, height, width, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor [%d, %d, %d, 3]" % (n, height, width))
    if (fill is not None or line is not None) and len(env.worlds) != 1:
        raise ValueError("explicit colour tables need a single-world env")
    for wi in np.unique(wis):
        pos = np.nonzero(wis == wi)[0]
        w = env.worlds[wi][0]
        f, l_ = (fill, line) if (fill is not None or line is not None) else _world_colors(env, wi)
        tabs = []
        for t in (f, l_):
            if t is not None:
                t = torch.as_tensor(t, dtype=torch.uint8, device=dev).contiguous()
                if tuple(t.shape) != (w.n_envs, w.lanes, 3):
                    raise ValueError("colour table must be uint8 [%d, %d, 3]" % (w.n_envs, w.lanes))
            tabs.append(t)
        idx = torch.as_tensor(loc[pos], dtype=torch.int32, device=dev)
        contiguous = len(pos) == int(pos[-1]) - int(pos[0]) + 1
        lo = int(pos[0])
        dst = out[lo:lo + len(pos)] if contiguous else torch.empty((len(pos), height, width, 3), dtype=torch.uint8, device=dev)
        cw = cam[lo:lo + len(pos)] if contiguous else cam[torch.as_tensor(pos, device=dev)].contiguous()
        _lib.check(w.L.rem2d_world_render(w.h, idx.data_ptr(), len(pos), cw.data_ptr(),
                                          tabs[0].data_ptr() if tabs[0] is not None else None,
                                          tabs[1].data_ptr() if tabs[1] is not None else None,
                                          width, height, dst.data_ptr(), w._stream()), w.wide)
        if not contiguous:
            out[torch.as_tensor(pos, device=dev)] = dst
    return out


def record_frames(env, steps, creatures=None, every=5, width=VIEWPORT_W, height=VIEWPORT_H, chunk=32, stop_when_frozen=True):
    """Steps ``env`` through ``steps`` env-steps and yields ``(step, frames)`` with frames uint8 numpy [n, H, W, 3] of the
    creatures before env-step ``step`` for every ``step % every == 0`` -- the frames the reference's evaluate() renders with
    INTERVAL = every (REM2D_main.py:363-365), under the reference's scrolling camera.  At most ``chunk`` frames live on the device
    at a time: they go to the host together.  With stop_when_frozen, the episode ends once every creature's fitness is final
    (the reference's ``break``)."""
    creatures = list(range(env.n_envs)) if creatures is None else list(creatures)
    n = len(creatures)
    dev = env.worlds[0][0].device
    cam = ReferenceCamera(n, dev)
    buf = torch.empty((chunk, n, height, width, 3), dtype=torch.uint8, device=dev)
    host = torch.empty(buf.shape, dtype=torch.uint8).pin_memory()
    held, stamps = 0, []

    def flush():
        host[:held].copy_(buf[:held])
        return [(s, host[k].numpy().copy()) for k, s in enumerate(stamps)]

    t = 0
    while True:
        render_frames(env, creatures, width, height, camera=cam, out=buf[held])
        stamps.append(t)
        held += 1
        if held == chunk:
            yield from flush()
            held, stamps = 0, []
        if t >= steps:
            break
        k = min(every, steps - t)
        if k > 1:   # (the scroll needs the root of the step before as well)
            env.step(k - 1)
            p = root_poses(env, creatures)
            cam.update(p[:, 0], p[:, 1])
        env.step(1)
        p = root_poses(env, creatures)
        cam.update(p[:, 0], p[:, 1])
        t += k
        if stop_when_frozen:
            frozen = env.frozen
            if bool((frozen[torch.as_tensor(creatures, device=frozen.device)] != 0).all()):
                break
    if held:
        yield from flush()


def write_png(frames, directory, prefix="frame", start=0):
    """Writes uint8 [n, H, W, 3] (or [H, W, 3]) frames as <prefix><k:05d>.png, k from ``start``; returns the paths."""
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    frames = _host(frames)
    if frames.ndim == 3:
        frames = frames[None]
    paths = []
    for k, f in enumerate(frames):
        path = os.path.join(directory, "%s%05d.png" % (prefix, start + k))
        Image.fromarray(f, "RGB").save(path, compress_level=1)
        paths.append(path)
    return paths


def write_npy(frames, path):
    """Writes uint8 frames as one .npy file; returns the path."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.save(path, _host(frames))
    return path


def _host(frames):
    if isinstance(frames, torch.Tensor):
        frames = frames.cpu().numpy()
    return np.ascontiguousarray(frames, dtype=np.uint8)
