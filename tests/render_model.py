"""numpy model of the renderer (gym_rem2d_amd/csrc/rem2d_raster.h), pixel for pixel.

Every quantity is binary32 and every operation is done in the kernel's order, each one rounded on its own (numpy float32
arithmetic never fuses), so a frame of the model equals the kernel's with ``np.array_equal``.  A body's rotation comes from
``oracle.sincosf``, the host twin of the engine's rot_set.
"""
import numpy as np

f32 = np.float32
INV = f32(1.0 / 30.0)
H2 = INV * INV
HALF = f32(0.5) * INV

SKY = (230, 230, 255)
GROUND = (102, 153, 76)
EDGE_EVEN, EDGE_ODD = (76, 255, 76), (76, 204, 76)
OBST_FILL, OBST_LINE = (255, 255, 255), (153, 153, 153)
WOD = (0, 0, 255)
FLAG_LINE, FLAG_FILL = (0, 0, 0), (230, 51, 0)
BOX_FILL, BOX_LINE = (127, 166, 217), (31, 63, 102)
CIRCLE_FILL, CIRCLE_LINE = (217, 166, 127), (102, 64, 31)

FLAG_X = f32(14.0 / 30.0 * 3.0)
FLAG_Y1 = f32(600.0 / 30.0 / 4.0)
FLAG_Y2 = f32(600.0 / 30.0 / 4.0 + 50.0 / 30.0)
FLAG_Y3 = f32(600.0 / 30.0 / 4.0 + 50.0 / 30.0 - 10.0 / 30.0)
FLAG_X2 = f32(14.0 / 30.0 * 3.0 + 25.0 / 30.0)
FLAG_Y4 = f32(600.0 / 30.0 / 4.0 + 50.0 / 30.0 - 5.0 / 30.0)


class Terrain:
    """What rem2d_world_set_terrain uploads: the polyline (xs, ys), the hardcore quads counter-clockwise (Box2D's hull order,
    up to a rotation of the vertex list, which no coverage test sees), x0 and 1 / pitch."""

    def __init__(self, xs, ys, polys=()):
        self.xs = np.asarray(xs, f32)
        self.ys = np.asarray(ys, f32)
        n_edge = len(self.xs) - 1
        pitch = (self.xs[-1] - self.xs[0]) / f32(n_edge)
        self.x0, self.inv_pitch, self.n_edge = self.xs[0], f32(1.0) / pitch, n_edge
        self.polys = []
        for q in np.asarray(polys, f32).reshape(-1, 4, 2):
            x, y = q[:, 0].astype(np.float64), q[:, 1].astype(np.float64)
            area = np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)
            self.polys.append(q if area > 0 else q[::-1].copy())

    @staticmethod
    def of(profile):
        xs, ys, polys = profile.f32()
        return Terrain(xs, ys, polys)


def _edge(ax, ay, dx, dy, X, Y):
    qx, qy = X - ax, Y - ay
    return dx * qy - dy * qx, dx * qx + dy * qy


def _band(cr, dt, len2, hh):
    return (cr * cr <= hh) & (dt >= f32(0)) & (dt <= len2)


def _segment(ax, ay, bx, by, X, Y):
    dx, dy = bx - ax, by - ay
    len2 = dx * dx + dy * dy
    cr, dt = _edge(ax, ay, dx, dy, X, Y)
    return _band(cr, dt, len2, H2 * len2)


def _poly(vx, vy, X, Y):
    """(fill, outline) masks of a convex CCW polygon."""
    n = len(vx)
    inside = np.ones(X.shape, bool)
    edge = np.zeros(X.shape, bool)
    for k in range(n):
        k1 = (k + 1) % n
        dx, dy = vx[k1] - vx[k], vy[k1] - vy[k]
        len2 = dx * dx + dy * dy
        cr, dt = _edge(vx[k], vy[k], dx, dy, X, Y)
        inside &= cr >= f32(0)
        edge |= _band(cr, dt, len2, H2 * len2)
    return inside & ~edge, edge


def box_vertices(px, py, ang, hx, hy, sincosf):
    s, c = (f32(v) for v in sincosf(f32(ang)))
    px, py, hx, hy = f32(px), f32(py), f32(hx), f32(hy)
    lx, ly = (-hx, hx, hx, -hx), (-hy, -hy, hy, hy)
    vx = [(c * lx[k] - s * ly[k]) + px for k in range(4)]
    vy = [(s * lx[k] + c * ly[k]) + py for k in range(4)]
    return vx, vy


def render(width, height, cam, terrain=None, bodies=(), fill=None, line=None, wod=None, flag=True, sincosf=None, brute=False):
    """uint8 [height, width, 3].  cam: (x, y) of the view's lower left corner; terrain: a :class:`Terrain` or None;
    bodies: (shape, px, py, angle, hx, hy) per slot (shape 0: none, 1: box, 2: circle); fill / line: rgb per slot or None
    for the shape colours; wod: the wall of death's x (a float64 state value) or None (not drawn); sincosf: oracle.sincosf.
    brute: the terrain without the kernel's shortcut -- every pixel is tested against EVERY edge (ground under each, then
    each edge line from the highest index down), with no edge index computed from the pixel's x; obstacles and bodies have no
    shortcut in either mode.  (The +-1 window of the other mode cannot cover a pitch under 2 px: a line's half width is 1 px.
    rem2d_world_set_terrain accepts such a pitch, no track has one, and nothing here draws one.)"""
    cx, cy = f32(cam[0]), f32(cam[1])
    i = np.arange(width, dtype=f32)
    j = np.arange(height, dtype=f32)
    X1 = cx + (i + f32(0.5)) * INV
    top = cy + f32(height) * INV
    Y1 = top - (j + f32(0.5)) * INV
    X, Y = np.meshgrid(X1, Y1)
    img = np.empty((height, width, 3), np.uint8)
    img[:] = SKY
    if terrain is not None and brute:
        for k in range(terrain.n_edge):
            ax, ay, bx, by = terrain.xs[k], terrain.ys[k], terrain.xs[k + 1], terrain.ys[k + 1]
            cr, _ = _edge(ax, ay, bx - ax, by - ay, X, Y)
            img[(X >= ax) & (X <= bx) & (Y >= f32(0)) & (cr <= f32(0))] = GROUND
        for k in range(terrain.n_edge - 1, -1, -1):
            m = _segment(terrain.xs[k], terrain.ys[k], terrain.xs[k + 1], terrain.ys[k + 1], X, Y)
            img[m] = EDGE_ODD if k & 1 else EDGE_EVEN
    elif terrain is not None:
        fi = (X1 - terrain.x0) * terrain.inv_pitch
        fi = np.where(fi < f32(-2), f32(-2), np.where(fi > f32(terrain.n_edge) + f32(1), f32(terrain.n_edge) + f32(1), fi))
        i0 = np.floor(fi).astype(np.int64)
        ne = terrain.n_edge

        def edge_of(off):
            k = i0 + off
            ok = (k >= 0) & (k < ne)
            kc = np.clip(k, 0, ne - 1)
            ax, ay, bx, by = terrain.xs[kc], terrain.ys[kc], terrain.xs[kc + 1], terrain.ys[kc + 1]
            return k, np.broadcast_to(ok, X.shape), ax, ay, bx, by
        for off in (-1, 0, 1):
            k, ok, ax, ay, bx, by = edge_of(off)
            cr, _ = _edge(ax, ay, bx - ax, by - ay, X, Y)
            img[ok & (X >= ax) & (X <= bx) & (Y >= f32(0)) & (cr <= f32(0))] = GROUND
        for off in (1, 0, -1):
            k, ok, ax, ay, bx, by = edge_of(off)
            m = ok & _segment(ax, ay, bx, by, X, Y)
            odd = np.broadcast_to((k & 1) == 1, X.shape)
            img[m & odd] = EDGE_ODD
            img[m & ~odd] = EDGE_EVEN
    if terrain is not None:
        for q in reversed(terrain.polys):
            fm, em = _poly(q[:, 0], q[:, 1], X, Y)
            img[fm] = OBST_FILL
            img[em] = OBST_LINE
    for slot, (shape, px, py, ang, hx, hy) in enumerate(bodies):
        if shape not in (1, 2):
            continue
        fc = fill[slot] if fill is not None else (CIRCLE_FILL if shape == 2 else BOX_FILL)
        lc = line[slot] if line is not None else (CIRCLE_LINE if shape == 2 else BOX_LINE)
        if shape == 2:
            r = f32(hx)
            ri, ro = r - INV, r + INV
            dx, dy = X - f32(px), Y - f32(py)
            d2 = dx * dx + dy * dy
            img[d2 <= r * r] = fc
            img[(d2 > ri * ri) & (d2 <= ro * ro)] = lc
        else:
            vx, vy = box_vertices(px, py, ang, hx, hy, sincosf)
            fm, em = _poly(vx, vy, X, Y)
            img[fm] = fc
            img[em] = lc
    if wod is not None:
        d = X - f32(wod)
        img[(d * d <= HALF * HALF) & (Y >= f32(-10)) & (Y <= f32(40))] = WOD
    if flag:
        img[_segment(FLAG_X, FLAG_Y1, FLAG_X, FLAG_Y2, X, Y)] = FLAG_LINE
        fm, em = _poly([FLAG_X, FLAG_X, FLAG_X2], [FLAG_Y2, FLAG_Y3, FLAG_Y4], X, Y)
        img[fm] = FLAG_FILL
        img[em] = FLAG_LINE
    return img
