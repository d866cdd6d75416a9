"""Scenes no genome and no production track puts in front of the renderer, shared by the host half
(tests/test_render_forge_host.py: keeps them from being vacuous) and the GPU half (tests/test_render_forge_gpu.py:
rem2d_world_render == the BRUTE pixel model, tests/render_model.render(brute=True), with np.array_equal, in all three builds).

The kernel reads shape, px, py, ang, hx, hy and wod straight from the state arena, and those views are writable, so a scene is
written there (``install``) and read back (``readback``) for the model: both sides see the same bits.

A scene is a terrain profile, the lane count, per creature and slot (shape, px, py, ang, hx, hy), a wall-of-death x per creature,
per-slot colour tables and a list of render calls (width, height, creature indices, view corners).  Bodies are laid out in PIXELS
of the view they are meant for (``xc`` / ``yc`` are the kernel's pixel-centre formula), so that vertices, centres and edges land
on pixel centres, tile seams and image borders on purpose.  Families:

  full64 / mixed64 / four   a 64-lane world with every slot drawn; the same with shape-0 gaps, a NaN px, a +inf py and a NaN
                            angle beside healthy slots, and a second creature under a box larger than the image; a 4-lane world.
                            Boxes at 0, pi/2, 1e-3, 0.7, pi/4 and 100 rad, hy of 0.4 and 1 px, discs of radius 0.5 px and exactly
                            1 px, a body on a tile corner, across every image border, and wholly outside within 2 px of it.
                            Each on the sawtooth (x about 10), on saw_coarse (x about 1000: a pixel is some 500 ulps of X) and on
                            saw_neg (x about -17, once with the whole view below y = 0).
  knife                     coverage ties: a 45 degree box with its vertices on pixel centres, 3-4-5 boxes and obstacle quads
                            (pixel centres at distance exactly 1 px of an edge), an axis-aligned box with its edges through
                            pixel centres, terrain edges of slope 1 and 3/4 through pixel centres.  There the separately rounded
                            products of cross(d, p - a) cancel or tie; an evaluation that fuses one product (``fused_edge``)
                            does not, which is what makes the three-build comparison bite.
  obst64 / obst65 / obst130 / obst130_70
                            overlapping obstacle boxes in shuffled index order over a flat polyline: 64 and 65 meeting one
                            64 x 16 tile (the list's last slot; the overflow path), 130 with no tile over 64 (three ballot
                            passes feeding one list), 130 with one tile seeing 70 (both paths in one image).
  shape_WxH                 image sizes at which the store paths change: widths below 4, = 2 mod 4, one past a tile, 1 x 1;
                            five images of two creatures in one call.
  terrain_<name>            every terrain of tests/terrain_forge.py under views over both ends, the steepest edge and a box.
"""
import math

import numpy as np

import render_model as M

f32 = np.float32
INV = M.INV
PX = 1.0 / 30.0
FIELDS = ("shape", "px", "py", "ang", "hx", "hy")
TILE_W, TILE_H, MAX_TILE_OBST = 64, 16, 64
B2_POLYGON_RADIUS, B2_AABB_EXTENSION = f32(2.0 * 0.005), f32(0.1)
W0, H0 = 256, 128                 # the largest image a scene uses
CONT = 1


def xc(cam_x, i):
    """the kernel's pixel-centre X of (possibly fractional or outside) pixel column i"""
    return f32(cam_x) + (f32(i) + f32(0.5)) * INV


def yc(cam_y, height, j):
    return (f32(cam_y) + f32(height) * INV) - (f32(j) + f32(0.5)) * INV


class Scene:
    def __init__(self, name, profile, lanes, creatures, wod, calls, seed=0):
        """creatures: per creature a list of <= lanes (shape, px, py, ang, hx, hy); calls: (width, height, [creature], [(x, y)])"""
        self.name, self.profile, self.lanes, self.calls = name, profile, lanes, calls
        n = self.n_envs = len(creatures)
        self.arrays = {k: np.zeros((n, lanes), np.int32 if k == "shape" else f32) for k in FIELDS}
        for e, bodies in enumerate(creatures):
            assert len(bodies) <= lanes
            for s, b in enumerate(bodies):
                for k, v in zip(FIELDS, b):
                    self.arrays[k][e, s] = v
        self.wod = np.asarray(wod, np.float64).reshape(n)
        rng = np.random.default_rng(1000 + seed)
        self.fill = rng.integers(0, 256, (n, lanes, 3)).astype(np.uint8)
        self.line = rng.integers(0, 256, (n, lanes, 3)).astype(np.uint8)
        assert all(w <= W0 and h <= H0 and len(c) == len(cams) for w, h, c, cams in calls)
        assert sum(len(c) for _, _, c, _ in calls) <= 8, name

    def state(self):
        """what `readback` returns when nothing was installed (the host half's input)"""
        return {k: v.copy() for k, v in self.arrays.items()}, self.wod.copy()


# ---------------------------------------------------------------------------------------------------------------- the model
def model_frames(scene, state, sincosf, brute=True, only=None):
    """[per call: uint8 [n, H, W, 3]] from the state `readback` (or `Scene.state`) returned"""
    arrays, wod = state
    T = M.Terrain.of(scene.profile)
    out = []
    with np.errstate(all="ignore"):        # (non-finite slots are part of the scenes)
        for ci, (w, h, creatures, cams) in enumerate(scene.calls):
            if only is not None and ci != only:
                continue
            frames = np.empty((len(creatures), h, w, 3), np.uint8)
            for k, (e, cam) in enumerate(zip(creatures, cams)):
                bodies = list(zip(*(arrays[f][e] for f in FIELDS)))
                frames[k] = M.render(w, h, cam, terrain=T, bodies=bodies, fill=scene.fill[e], line=scene.line[e], wod=wod[e],
                                     sincosf=sincosf, brute=brute)
            out.append(frames)
    return out


def fused_edge(which):
    """render_model._edge as a contracting compiler may evaluate it: one product of each sum exact (the binary64 product of two
    binary32 numbers), the other rounded to binary32, the sum rounded once.  which = 0 / 1: the first / second product is the
    fused one."""
    d = np.float64

    def _edge(ax, ay, dx, dy, X, Y):
        qx, qy = X - ax, Y - ay
        a, b = (dx * qy, dy * qx)
        c, e = (dx * qx, dy * qy)
        if which == 0:
            cr = d(dx) * qy.astype(d) - b.astype(d)
            dt = d(dx) * qx.astype(d) + e.astype(d)
        else:
            cr = a.astype(d) - d(dy) * qx.astype(d)
            dt = c.astype(d) + d(dy) * qy.astype(d)
        return cr.astype(f32), dt.astype(f32)
    return _edge


def colour_mask(img, rgb):
    return np.all(img == np.array(rgb, np.uint8), axis=-1)


# ------------------------------------------------------------------------------------------------- the obstacle list per tile
def fat_aabbs(profile):
    """(flx, fly, fux, fuy) of every obstacle as rem2d_world_set_terrain computes them, binary32"""
    q = profile.f32()[2].reshape(-1, 4, 2)
    lx, ly, ux, uy = q[:, :, 0].min(1), q[:, :, 1].min(1), q[:, :, 0].max(1), q[:, :, 1].max(1)
    r, x = B2_POLYGON_RADIUS, B2_AABB_EXTENSION
    return (lx - r) - x, (ly - r) - x, (ux + r) + x, (uy + r) + x


def tile_lists(profile, cam, width, height):
    """{(ty, tx): obstacle indices whose fat AABB meets the tile's pixel-centre span}: the kernel's own rule"""
    flx, fly, fux, fuy = fat_aabbs(profile)
    out = {}
    for ty in range((height + TILE_H - 1) // TILE_H):
        for tx in range((width + TILE_W - 1) // TILE_W):
            i0, j0 = tx * TILE_W, ty * TILE_H
            i1, j1 = min(i0 + TILE_W, width) - 1, min(j0 + TILE_H, height) - 1
            lX, uX = xc(cam[0], i0), xc(cam[0], i1)
            uY, lY = yc(cam[1], height, j0), yc(cam[1], height, j1)
            out[ty, tx] = np.nonzero((fux >= lX) & (flx <= uX) & (fuy >= lY) & (fly <= uY))[0]
    return out


# --------------------------------------------------------------------------------------------------------------------- bodies
def _T():
    from gym_rem2d_amd import terrain
    return terrain


def _flat(x0, x1, y):
    T = _T()
    n = int(math.ceil((x1 - x0) / T.TERRAIN_STEP)) + 1
    return x0 + T.TERRAIN_STEP * np.arange(n), np.full(n, y)


def zoo(cam, kind):
    """bodies of one creature laid out for a W0 x H0 view at `cam`; kind: full64 | mixed64 | big | four"""
    cx, cy = cam

    def box(i, j, ang, hx, hy):
        return (1, xc(cx, i), yc(cy, H0, j), f32(ang), f32(hx * PX), f32(hy * PX))

    def disc(i, j, r):
        return (2, xc(cx, i), yc(cy, H0, j), f32(0.3), f32(r * PX) if r != 1 else INV, f32(0))
    if kind == "four":
        return [box(40, 40, 0.7, 20, 8), (0, 0, 0, 0, 0, 0), disc(70, 50, 12), box(60, 44, 0.3, 30, 0.4)]
    if kind == "big":
        return [box(128, 64, 0.2, 180, 120), disc(100, 60, 20), (0, 0, 0, 0, 0, 0), box(150, 70, 2.0, 30, 10)]
    b = [box(30, 30, 0.0, 20, 8), box(60, 40, math.pi / 2, 20, 8), box(95, 28, 1e-3, 20, 8), box(130, 35, 0.7, 20, 8),
         box(165, 30, math.pi / 4, 20, 8), box(200, 35, 100.0, 20, 8),
         box(40, 70, 0.3, 25, 0.4), box(40, 85, 0.0, 25, 1.0), box(100, 85, 0.0, 25, 0.4), box(100.3, 90.4, 1.2, 25, 1.0),
         disc(120, 70, 0.5), disc(125.3, 70.4, 0.5), disc(135, 70, 1), disc(140.5, 70.5, 1),
         disc(-6, 60, 15),                                    # the centre outside the image
         disc(64, 16, 6), box(127.5, 31.5, 0.4, 9, 5),       # on a tile's first pixel; on the corner four tiles share
         box(0, 100, 0.5, 12, 6), box(255, 50, -0.4, 12, 6), box(200, 0, 0.9, 12, 6), box(80, 127, 0.1, 12, 6),   # across each border
         disc(255.5, 127.5, 9), box(-0.5, -0.5, 0.78, 10, 10),                                                  # across two corners
         box(-10.9, 40, 0.0, 10, 6),      # wholly outside, its outline reaches the first pixel column (edge 0.9 px from its centres)
         box(120, -7.5, 0.0, 10, 6),      # wholly outside by 1.5 px: listed by the cull, paints nothing
         disc(150, 127 + 8.7, 8)]         # centre and disc outside, the ring reaches the last row
    rng = np.random.default_rng(7)
    while len(b) < 64:                     # a crowd of overlapping small bodies in the lower right
        i, j = rng.uniform(150, 250), rng.uniform(60, 120)
        b.append(disc(i, j, rng.uniform(2, 9)) if len(b) % 3 == 0 else box(i, j, rng.uniform(-4, 4), rng.uniform(2, 14), rng.uniform(1, 7)))
    if kind == "mixed64":
        for s in (3, 26, 27, 40, 63):
            b[s] = (0,) + b[s][1:]
        nan, inf = f32("nan"), f32("inf")
        b[30] = (1, nan) + b[30][2:]                          # NaN px (a box, over the crowd)
        b[31] = (2, b[31][1], inf) + b[31][3:]                # +inf py
        b[32] = (1, b[32][1], b[32][2], nan) + b[32][4:]      # NaN angle
        b[33] = (2, nan) + b[33][2:]
        b[35] = (1, b[35][1], inf) + b[35][3:]
    else:
        assert kind == "full64"
    return b


NONFINITE_SLOTS = (30, 31, 32, 33, 35)

# (terrain of tests/terrain_forge.py, view corners): x about 10, about 1000, negative x, negative x and y
ORIGINS = {"near": ("saw", [(10.3, 7.2)]), "far": ("saw_coarse", [(1003.1, 7.2)]), "neg": ("saw_neg", [(-17.3, 6.9), (-17.3, -6.0)])}


def body_scenes():
    import terrain_forge as TF
    out = []
    for oname, (tname, cams) in ORIGINS.items():
        prof = TF.profile(tname)
        for kind in ("full64", "mixed64", "four"):
            creatures = [zoo(cam, kind) for cam in cams]
            idx = list(range(len(cams)))
            wod = [cam[0] + 100.5 * PX for cam in cams]
            views = list(cams)
            if kind == "mixed64":
                creatures.append(zoo(cams[0], "big"))
                idx.append(len(cams))
                wod.append(cams[0][0] - 3.0)
                views.append(cams[0])
            out.append(Scene("%s_%s" % (kind, oname), prof, 4 if kind == "four" else 64, creatures, wod,
                             [(W0, H0, idx, views)], seed=len(out)))
    return out


# ---------------------------------------------------------------------------------------------------------------- knife edges
KNIFE_CAM = (0.25, 4.0)
KNIFE_SHIFTS = ((0, 0), (69, 4), (40, 7), (9, -8), (74, 4), (40, -4), (50, 0), (10, 1))
KNIFE_END = (13, 5)                # the polyline's point count and last rise: it ends on a pixel centre inside the first view


def _quad_px(cam, i, j, pts):
    return [[xc(cam[0], i + a), yc(cam[1], H0, j - b)] for a, b in pts]          # (b upwards: CCW stays CCW)


def knife_scene():
    T = _T()
    cam = KNIFE_CAM
    # polyline through pixel centres, 20 px pitch: slopes 3/4, 1 and 0 both ways
    rises, ix, jy, j = (15, -15, 15, -15, 0, 20, -20, 15, -15, -15, 15), [], [], 116
    for k in range(KNIFE_END[0]):
        ix.append(-110 + 20 * k)
        jy.append(j)
        j -= rises[k % 11] if k < KNIFE_END[0] - 2 else KNIFE_END[1]
    xs, ys = [xc(cam[0], i) for i in ix], [yc(cam[1], H0, j) for j in jy]
    # 3-4-5 quads with their vertices on pixel centres (sides 25 and 20 px), overlapping, and an axis-aligned one
    r345 = [(0, 0), (20, 15), (5, 35), (-15, 20)]
    polys = [_quad_px(cam, 60, 80, r345), _quad_px(cam, 72, 74, r345), _quad_px(cam, 150, 90, [(0, 0), (24, 0), (24, 10), (0, 10)]),
             _quad_px(cam, 200, 50, [(0, 0), (12, 16), (-4, 28), (-16, 12)]), _quad_px(cam, 290, 70, r345), _quad_px(cam, 330, 110, r345)]
    prof = T.TerrainProfile(np.array(xs, np.float64), np.array(ys, np.float64), np.array(polys, np.float64))
    cx, cy = cam
    a345 = math.atan2(3.0, 4.0)

    def box(i, j, ang, hx, hy):
        return (1, xc(cx, i), yc(cy, H0, j), f32(ang), f32(hx * PX), f32(hy * PX))
    r2 = math.sqrt(0.5)
    bodies = [box(40, 30, math.pi / 4, 12 * r2, 12 * r2),       # vertices 12 px from the centre along the axes
              box(90, 30, math.pi / 4, 20 * r2, 6 * r2),
              box(140, 26, a345, 10, 5), box(150, 30, a345, 10, 5),          # vertices (+-5, +-10), (+-11, +-2) px from the centre
              box(200, 28, a345 + math.pi / 2, 20, 10),
              box(40, 64.5, 0.0, 15.5, 6),                                    # the four edges on pixel BOUNDARIES
              box(100, 60, 0.0, 10, 4), box(230, 100, math.pi / 2, 10, 4),    # the four edges through pixel centres
              (2, xc(cx, 120), yc(cy, H0, 60), f32(0), f32(5 * PX), f32(0)),  # d^2 ties: pixels (3, 4) px from the centre
              box(180.5, 40.5, -a345, 12.5, 7.5), box(300, 40, a345, 20, 10), box(340, 60, -a345, 10, 5)]
    # eight views a whole number of pixels apart (up to rounding: every view has its own near-ties)
    cams = [(float(f32(cx + a * PX)), float(f32(cy + b * PX))) for a, b in KNIFE_SHIFTS]
    return Scene("knife", prof, 16, [bodies], [cx + 100.5 * PX], [(W0, H0, [0] * len(cams), cams)], seed=50)


# ------------------------------------------------------------------------------------------------------------------ obstacles
OBST_CAM = (0.2, 4.0)
OBST_TILE = (1, 1)                 # (ty, tx): pixels 64..127 x 16..31


def _boxes_px(cam, items, order_seed):
    """items: (i, j, half width, half height, angle) in pixels -> quads [n][4][2] float64, indices shuffled"""
    quads = []
    for i, j, hw, hh, ang in items:
        c, s = math.cos(ang), math.sin(ang)
        x0, y0 = float(xc(cam[0], i)), float(yc(cam[1], H0, j))
        quads.append([[x0 + (c * a - s * b) * PX, y0 + (s * a + c * b) * PX] for a, b in ((-hw, -hh), (hw, -hh), (hw, hh), (-hw, hh))])
    quads = np.array(quads, np.float64)
    return quads[np.random.default_rng(order_seed).permutation(len(quads))]


def _in_tile(n_cols, n_rows, hw, hh):
    """n_cols x n_rows overlapping boxes inside tile OBST_TILE, every third one tilted"""
    items = []
    for b in range(n_rows):
        for a in range(n_cols):
            i = 64 + 5 + (54.0 * a) / (n_cols - 1)
            j = 16 + 3.5 + (9.0 * b) / (n_rows - 1)
            k = len(items)
            items.append((i, j, hw + (k % 4), hh + (k % 3) * 0.5, 0.0 if k % 3 else 0.35))
    return items


def _spread(n_cols, n_rows, hw, hh, skip=None):
    items = []
    for b in range(n_rows):
        for a in range(n_cols):
            i, j = 4 + (W0 - 8.0) * a / (n_cols - 1), 6 + (H0 - 30.0) * b / (n_rows - 1)
            if skip is not None and skip(i, j):
                continue
            k = len(items)
            items.append((i, j, hw + (k % 3), hh + (k % 2), 0.0 if k % 4 else -0.5))
    return items


def obstacle_scenes():
    T = _T()
    cam = OBST_CAM
    xs, ys = _flat(-2.0, 12.0, 4.6)
    sets = {
        "obst64": _in_tile(16, 4, 5, 3),
        "obst65": _in_tile(16, 4, 5, 3) + [(96, 24, 3, 3, 0.2)],
        "obst130": _spread(26, 5, 7, 8),
        "obst130_70": _in_tile(14, 5, 3, 2) + _spread(14, 7, 8, 5, skip=lambda i, j: 40 < i < 150 and j < 50)[:60],
    }
    out = []
    for k, (name, items) in enumerate(sets.items()):
        prof = T.TerrainProfile(xs, ys, _boxes_px(cam, items, 20 + k))
        cx, cy = cam
        bodies = [(1, xc(cx, 90), yc(cy, H0, 22), f32(0.4), f32(14 * PX), f32(4 * PX)), (2, xc(cx, 20), yc(cy, H0, 100), f32(0), f32(9 * PX), f32(0))]
        out.append(Scene(name, prof, 4, [bodies], [cx + 30.5 * PX], [(W0, H0, [0], [cam])], seed=60 + k))
    return out


def swapped(profile, a, b):
    """the profile with obstacles a and b exchanged in the index order"""
    q = profile.polys.copy()
    q[[a, b]] = q[[b, a]]
    return _T().TerrainProfile(profile.xs, profile.ys, q, profile.friction)


# --------------------------------------------------------------------------------------------------------------------- shapes
SIZES = ((1, 1), (2, 1), (3, 2), (4, 1), (5, 17), (6, 3), (64, 16), (65, 17), (66, 33), (70, 16), (255, 2))
SHAPE_CAM = (35.0, 4.0)


def _shape_creatures(x0, top):
    """two creatures laid out from the view's TOP LEFT corner (x0, top), which every size shares"""
    def box(i, j, ang, hx, hy):
        return (1, x0 + (i + 0.5) * PX, top - (j + 0.5) * PX, f32(ang), f32(hx * PX), f32(hy * PX))

    def disc(i, j, r):
        return (2, x0 + (i + 0.5) * PX, top - (j + 0.5) * PX, f32(0), f32(r * PX), f32(0))
    one = [box(1, 0, 0.6, 3, 1.2), disc(4, 1, 1.6), box(40, 9, -0.3, 30, 5), disc(64, 16, 5), box(200, 1, 0.05, 60, 0.4), disc(66, 30, 4)]
    two = [disc(0, 0, 2.2), box(3, 2, 1.0, 2.5, 0.8), box(64.5, 8, 0.9, 12, 3), disc(250, 1, 3)]
    return [one, two]


def shape_scenes():
    """every size with n = 1 and, up to 70 x 16, with n = 5 (two creatures, repeated, under four cameras); n = 0 is the GPU
    half's own test.  The view's top left corner is fixed (cam_y follows the height), so every size looks at the same bodies."""
    import terrain_forge as TF
    prof = TF.profile("hardcore0")
    out = []
    x0, top = SHAPE_CAM[0], SHAPE_CAM[1] + 40 * PX
    cr = _shape_creatures(x0, top)
    for k, (w, h) in enumerate(SIZES):
        cam = (x0, float(f32(top - h * PX)))
        calls = [(w, h, [0], [cam])]
        if w * h <= 70 * 16:
            dx = [(0.0, 0.0), (1.0 * PX, 0.0), (0.4 * PX, -0.3 * PX), (-2.0 * PX, 1.0 * PX), (0.0, 0.0)]
            calls.append((w, h, [1, 0, 1, 1, 0], [(cam[0] + a, cam[1] + b) for a, b in dx]))
        out.append(Scene("shape_%dx%d" % (w, h), prof, 8, cr, [x0 + 2.5 * PX, x0 + 5.5 * PX], calls, seed=80 + k))
    return out


# ------------------------------------------------------------------------------------------------------------------- terrains
def terrain_views(prof, width=W0, height=H0):
    """view corners over the track's two ends, its steepest edge, the middle and (hardcore) a box"""
    xs, ys = np.asarray(prof.xs), np.asarray(prof.ys)
    vw, vh = width * PX, height * PX
    k = int(np.argmax(np.abs(np.diff(ys) / np.diff(xs))))
    m = len(xs) // 2
    cams = [(xs[0] - 0.3 * vw, ys[0] - 0.5 * vh), (xs[-1] - 0.7 * vw, ys[-1] - 0.5 * vh),
            (0.5 * (xs[k] + xs[k + 1]) - 0.5 * vw, 0.5 * (ys[k] + ys[k + 1]) - 0.5 * vh), (xs[m] - 0.5 * vw, ys[m] - 0.6 * vh)]
    if len(prof.polys):
        q = prof.polys[len(prof.polys) // 2]
        cams.append((q[:, 0].mean() - 0.45 * vw, q[:, 1].mean() - 0.5 * vh))
    return [(float(f32(a)), float(f32(b))) for a, b in cams]


def terrain_scenes():
    import terrain_forge as TF
    out = []
    for k, name in enumerate(TF.TERRAINS):
        prof = TF.profile(name)
        cams = terrain_views(prof)
        creatures = [zoo(cam, "four") for cam in cams]
        out.append(Scene("terrain_" + name, prof, 4, creatures, [cam[0] + 200.5 * PX for cam in cams],
                         [(W0, H0, list(range(len(cams))), cams)], seed=100 + k))
    return out


_SCENES = {}


def scenes():
    """name -> Scene, every family"""
    if not _SCENES:
        for s in body_scenes() + [knife_scene()] + obstacle_scenes() + shape_scenes() + terrain_scenes():
            assert s.name not in _SCENES
            _SCENES[s.name] = s
    return _SCENES


def names():
    import terrain_forge as TF
    return (["%s_%s" % (k, o) for o in ORIGINS for k in ("full64", "mixed64", "four")] + ["knife", "obst64", "obst65", "obst130", "obst130_70"]
            + ["shape_%dx%d" % s for s in SIZES] + ["terrain_" + n for n in TF.TERRAINS])


# -------------------------------------------------------------------------------------------------------------- the GPU side
def install(scene, wide=False):
    """A BatchedWorld of the scene's build holding the scene: set_terrain, reset with a chain population, then the views and wod
    overwritten.  -> (world, fill table, line table) on the device"""
    import torch
    from gym_rem2d_amd import synthetic
    from gym_rem2d_amd.world import BatchedWorld
    w = BatchedWorld(scene.n_envs, scene.lanes, CONT, wide=wide)
    w.set_terrain(scene.profile)
    w.reset(synthetic.chain_population(scene.n_envs, 4, "left", lanes=scene.lanes))
    for k in FIELDS:
        w.view(k)[:] = torch.from_numpy(scene.arrays[k]).to(w.device)
    w.view("wod")[:] = torch.from_numpy(scene.wod).to(w.device)
    return w, torch.from_numpy(scene.fill).to(w.device), torch.from_numpy(scene.line).to(w.device)


def readback(w):
    return {k: w.view(k).cpu().numpy().copy() for k in FIELDS}, w.view("wod").cpu().numpy().astype(np.float64).copy()


def same_state(a, b):
    return all(np.array_equal(a[0][k].view(np.uint32), b[0][k].view(np.uint32)) for k in FIELDS) and np.array_equal(a[1], b[1])


def render_call(w, creatures, cams, width, height, fill=None, line=None, out=None):
    """rem2d_world_render straight through the library; out: a uint8 device tensor of n * H * W * 3 elements (any alignment)"""
    import torch
    from gym_rem2d_amd import _lib
    n = len(creatures)
    idx = torch.tensor(list(creatures), dtype=torch.int32, device=w.device)
    cam = torch.tensor(np.asarray(cams, f32).reshape(n, 2), dtype=torch.float32, device=w.device)
    if out is None:
        out = torch.full((n, height, width, 3), 0x5A, dtype=torch.uint8, device=w.device)
    assert out.numel() == n * height * width * 3 and out.is_contiguous()
    _lib.check(w.L.rem2d_world_render(w.h, idx.data_ptr(), n, cam.data_ptr(), fill.data_ptr() if fill is not None else None,
                                      line.data_ptr() if line is not None else None, width, height, out.data_ptr(), w._stream()), w.wide)
    return out
