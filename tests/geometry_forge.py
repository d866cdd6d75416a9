"""Pairs of shapes the dynamics never choose: the cases of the collision-geometry self-test, shared by the host half
(tests/test_geometry_forge_host.py, the oracle alone) and the GPU half (tests/test_geometry_gpu.py, rem2d_selftest_geometry against
rem2d_oracle_kat_geometry_batch).

Everything the step kernels know about contact comes from six device functions -- collide_edge_circle, collide_edge_box,
collide_polygons, collide_polygon_circle (csrc/rem2d_narrowphase.h), gjk_distance and time_of_impact (csrc/rem2d_toi.h) -- and
one early-out with no oracle counterpart, toi_far_apart.  The places where such routines go wrong (a separation exactly at a
radius, a tie between two faces, a vertex on a line) have measure zero on a trajectory; here they are the inputs.

A case is one static shape A at the identity (an isolated terrain edge, or a hardcore box) and one module shape B (box or circle)
at a pose (collide, distance) or over a sweep (toi, far_apart): ORACLE_WORDS binary32 words, the table
rem2d_oracle_kat_geometry_batch reads; `device_table` turns it into the device's (a hardcore box becomes the vertices and normals
the library's own terrain code derives).  Deterministic, numpy only; every input is computed in binary64 and rounded ONCE to
binary32, so oracle and device receive the same bits.  A boundary ("exactly at ...") is a LADDER: the binary64 position of the
boundary rounded to binary32, and the binary32 neighbours k ulps either side, so that wherever the binary32 arithmetic under
test puts the change of outcome, two neighbouring steps of the ladder stand either side of it: the steps run along the
direction that crosses the boundary, one ulp of the LARGER coordinate apart, 16 either side (LADDER_K says why 16).  The host
half asserts that the outcome changes inside EVERY ladder (1 672 contact-radius ladders, 88 flip-rule ladders) and inside
none of the same ladders moved off the boundary (5 mm; 2 cm for the flip rule).  Boundaries that binary32 can meet to the
bit are also met to the bit: `ec/dd_eq_rr`, `bb/flip_tie`, and the exact zeros the host half counts.

Shapes: the module classes' boxes (half-extents 0.25 .. 0.5), 0.2 x 0.8, one thin plank, circles 0.25 / 0.37 / 0.5; edges of the
reference pitch 14 / 30 with slopes 0, +-0.05 .. +-2.7 and a vertical riser; hardcore boxes as terrain.py makes them for the
seed-4 hardcore track.  Every family runs at x = 0 .. 93 and once more translated to x = 1000 (one ulp there: 6e-5).
"""
import numpy as np

f32, f64 = np.float32, np.float64
ORACLE_WORDS = 18
DEVICE_WORDS = 26
OUT_WORDS = 8
PITCH = 14.0 / 30.0
SLOP = 0.005
POLY_R = 2 * SLOP
TOL = 0.25 * SLOP
BOXES = ((0.25, 0.25), (0.5, 0.5), (0.25, 0.4), (0.1, 0.4), (0.5, 0.025))       # smallest, largest, default, 0.2 x 0.8, plank
CIRCLES = (0.25, 0.5, 0.37)
SLOPES = (0.0, 0.05, -0.05, 0.3, -0.3, 1.0, -1.0, 2.7, -2.7)
OFFSETS = (0.0, 1000.0)
TOI_STATES = ("unknown", "failed", "overlapped", "touching", "separated")


def toi_target(body):
    """b2TimeOfImpact's target distance of the core shapes for a module body against a static shape."""
    total = POLY_R + (POLY_R if body[0] == 1 else body[1])
    return max(SLOP, total - 3 * SLOP)


def need_of(body):
    return toi_target(body) + TOL


def ladder(x, k):
    """x rounded to binary32 and its neighbours -k .. +k ulps away, ascending."""
    x = f32(x)
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo = np.nextafter(lo, f32(-np.inf))
        hi = np.nextafter(hi, f32(np.inf))
        out = [lo] + out + [hi]
    return [float(v) for v in out]


# ---- static shapes and frames -----------------------------------------------------------------------------------------
class Static:
    """kind 0: an edge a -> b; kind 1: a hardcore box (raw: the four corners as the terrain lists them).  frames: (a, b) pairs
    in binary64 of the binary32 geometry, each with its outward ("up") normal u = (-e.y, e.x): the edge itself, or the box's
    top, right and left faces."""

    def __init__(self, kind, raw, name):
        self.kind, self.name = kind, name
        self.raw = np.zeros(8, f32)
        self.raw[:len(raw)] = np.asarray(raw, f64).astype(f32)
        self.rawlist = [float(v) for v in self.raw]
        r = self.raw.astype(f64)
        if kind == 0:
            self.frames = [(r[0:2], r[2:4])]
        else:
            xs, ys = r[0::2], r[1::2]
            x0, x1, y0, y1 = xs.min(), xs.max(), ys.min(), ys.max()
            self.frames = [(np.array([x0, y1]), np.array([x1, y1])), (np.array([x1, y1]), np.array([x1, y0])),
                           (np.array([x0, y0]), np.array([x0, y1]))]


def edges(offset):
    out = []
    for i, s in enumerate(SLOPES):
        x0 = offset + PITCH * (7 + 21 * i)            # 3.3 .. 81.7: over the length of the track
        out.append(Static(0, [x0, 5.0, x0 + PITCH, 5.0 + s * PITCH], "edge%+.2f" % s))
    xr = offset + PITCH * 199                          # x = 92.9
    out.append(Static(0, [xr, 5.0, xr, 5.5], "riser"))
    return out


_POLYS = []


def _hardcore_polys():
    if not _POLYS:
        from gym_rem2d_amd import make_terrain
        _POLYS.append(make_terrain(4, hardcore=True).polys)
    return _POLYS[0]


def hardcore_boxes(offset):
    """One box of every distinct size on the seed-4 hardcore track, corners in terrain.py's order."""
    polys = _hardcore_polys()
    seen, out = set(), []
    for p in polys:
        size = (round(float(np.ptp(p[:, 0])), 4), round(float(np.ptp(p[:, 1])), 4))
        if size in seen:
            continue
        seen.add(size)
        q = p.copy()
        q[:, 0] += offset
        out.append(Static(1, q.reshape(8), "box%gx%g" % size))
    return out[:4]


def statics(offset):
    return edges(offset) + hardcore_boxes(offset)


def bodies():
    return [(1, hx, hy) for hx, hy in BOXES] + [(2, r, 0.0) for r in CIRCLES]


def frame(a, b):
    e = (b - a) / np.hypot(*(b - a))
    return e, np.array([-e[1], e[0]]), float(np.arctan2(e[1], e[0]))


def extent(body, phi):
    """How far the core of the body reaches towards the frame's face when turned by phi against it."""
    if body[0] == 2:
        return 0.0
    return body[1] * abs(np.sin(phi)) + body[2] * abs(np.cos(phi))


class Table:
    def __init__(self):
        self.rows, self.family = [], []

    def add(self, fam, st, body, c0, a0, c=None, a=None):
        c = c0 if c is None else c
        a = a0 if a is None else a
        self.rows.append([st.kind, *st.rawlist, body[0], body[1], body[2], c0[0], c0[1], a0, c[0], c[1], a])
        self.family.append(fam)

    def place(self, fam, st, fr, body, s, sep, phi, dy_ulps=0):
        """B over frame fr of st: centre at fraction s along the face, its core `sep` above the face line, turned by phi."""
        a, b = fr
        e, u, ang = frame(a, b)
        c = a + s * (b - a) + (extent(body, phi) + sep) * u
        if dy_ulps:
            c = np.array([float(f32(c[0])), ladder(c[1], abs(dy_ulps))[abs(dy_ulps) + dy_ulps]])
        self.add(fam, st, body, c, ang + phi)

    def ladder(self, fam, st, body, c, direction, ang, k=None):
        k = LADDER_K if k is None else k
        c = np.asarray(c, f64)
        step = float(np.spacing(f32(max(abs(c[0]), abs(c[1])))))
        for j in range(-k, k + 1):
            self.add(fam, st, body, c + j * step * np.asarray(direction, f64), ang)

    def done(self):
        spec = np.asarray(self.rows, f64).astype(f32)
        assert spec.shape[1] == ORACLE_WORDS and np.isfinite(spec).all()
        fam = np.asarray(self.family)
        return spec, fam


def _kindname(st, body):
    return ("e" if st.kind == 0 else "b") + ("b" if body[0] == 1 else "c")      # eb ec bb bc


# ---- collide ---------------------------------------------------------------------------------------------------------------
# A boundary ladder: 2 K + 1 centres along the direction that crosses the boundary, one ulp of the LARGER coordinate apart, each
# coordinate rounded to binary32, so neighbouring steps differ by at most one ulp in either coordinate.  K from the arithmetic under
# test: a separation is a handful of separately rounded binary32 operations on coordinates of magnitude M (transform of a vertex,
# a difference, a dot product with a unit normal: each result rounded by at most half an ulp of M, the inputs by another half),
# so the binary32 outcome changes within some 5 ulp(M) of the binary64 boundary; 16 leaves a factor of three.  The controls stand
# CONTROL_SHIFT off the boundary: more than 16 ulp at x = 1000 (1 mm).
LADDER_K = 16
CONTROL_SHIFT = 5e-3


def collide_cases():
    """(spec, family): family names are '<pair>/<family>@<offset>' with pair in eb ec bb bc; ladders are
    '<pair>/<what>#<id>@<offset>' (one id per ladder, steps in ascending order) and their controls off the boundary '...~<id>'."""
    T = Table()
    lid = 0
    for off in OFFSETS:
        tag = "@%g" % off
        for st in statics(off):
            for body in bodies():
                pair = _kindname(st, body)
                box = body[0] == 1
                rad = POLY_R + (POLY_R if box else body[1])             # the contact radius of the pair
                for fi, fr in enumerate(st.frames):
                    # flat on the face / regions: along the face and beyond both ends, above and under it, five depths
                    for s in (-0.6, -0.05, 0.0, 0.3, 0.5, 1.0, 1.05, 1.6):
                        for sep in (-0.08, -0.01, 0.0, 0.5 * rad, rad - 1e-4, rad + 1e-3):
                            T.place(pair + "/regions" + tag, st, fr, body, s, sep, 0.0)
                    if st.kind == 0:      # edges are two-sided: the body under the edge
                        e, u, ang = frame(*fr)
                        for s in (0.0, 0.5, 1.2):
                            for sep in (-0.01, 0.5 * rad, rad + 1e-3):
                                c = fr[0] + s * (fr[1] - fr[0]) - (extent(body, 0.3) + sep) * u
                                T.add(pair + "/under" + tag, st, body, c, ang + 0.3)
                    # the centre on the face's line (inside a hardcore box's skin), and well inside a box
                    for s in (-0.2, 0.0, 0.5, 1.0, 1.2):
                        T.place(pair + "/online" + tag, st, fr, body, s, -extent(body, 0.0), 0.0)
                    if st.kind == 1 and fi == 0:
                        xs, ys = st.raw[0::2].astype(f64), st.raw[1::2].astype(f64)
                        for fx in (0.02, 0.5, 0.98):
                            for fy in (0.02, 0.5, 0.98):
                                c = (xs.min() + fx * np.ptp(xs), ys.min() + fy * np.ptp(ys))
                                T.add(pair + "/inside" + tag, st, body, c, 0.4 * fx)
                    # the contact radius exactly: ladders over the face, past the end (vertex region) and turned by 0.3
                    for s, phi in ((0.5, 0.0), (1.0, 0.0), (0.0, 0.0), (0.5, 0.3)) + (((1.3, 0.0), (-0.3, 0.0)) if not box else ()):
                        e, u, ang = frame(*fr)
                        for ctl, shift in (("#", 0.0), ("~", CONTROL_SHIFT)):
                            if s in (1.3, -0.3):   # a circle beyond the end: its centre `rad` from the end point, along the face
                                step = e if s > 1 else -e
                                c = (fr[1] if s > 1 else fr[0]) + (rad + shift) * step
                                T.ladder("%s/radius%s%d%s" % (pair, ctl, lid, tag), st, body, c, step, ang)
                            else:
                                c = fr[0] + s * (fr[1] - fr[0]) + (extent(body, phi) + rad + shift) * u
                                if box and phi > 0:    # the turned box's low corner over that point of the face, not its centre
                                    c = c - (-body[1] * np.cos(phi) + body[2] * np.sin(phi)) * e
                                T.ladder("%s/radius%s%d%s" % (pair, ctl, lid, tag), st, body, c, u, ang + phi)
                        lid += 1
                    if box:
                        # angles at exact multiples of pi / 4 and one ulp either side (the incident-edge tie at 45 degrees)
                        for m in range(8):
                            for ang_rel in ladder(m * np.pi / 4, 1):
                                T.place(pair + "/angle" + tag, st, fr, body, 0.5, 0.25 * rad, ang_rel)
                                T.place(pair + "/angle" + tag, st, fr, body, 1.0, 0.25 * rad, ang_rel)
                        # a corner over either end point, corner to corner
                        for s in (0.0, 1.0):
                            for ds in (-0.02, 0.0, 0.02):
                                for sep in (-0.02, 0.25 * rad, rad - 1e-4):
                                    T.place(pair + "/corner" + tag, st, fr, body, s + ds, sep, np.arctan2(body[2], body[1]))
                                    T.place(pair + "/corner" + tag, st, fr, body, s + ds, sep, np.pi / 4)
                        # depth sweep across the choice of the reference face (k_relativeTol / k_absoluteTol, the flip rule):
                        # the box hangs over an end, tilted, from 0.2 m deep to just out of reach
                        for s in (0.9, 1.15, -0.1):
                            for phi in (0.08, -0.3, 0.8):
                                for sep in np.linspace(-0.2, rad + 0.002, 24):
                                    T.place(pair + "/depth" + tag, st, fr, body, s, float(sep), phi)
                        # clips that keep two, one and zero points: along the face and off both ends
                        for phi in (0.0, 0.2):
                            for s in np.linspace(-1.5, 2.5, 33):
                                T.place(pair + "/clip" + tag, st, fr, body, float(s), 0.25 * rad, phi)
            # the flip rule's boundary, box on hardcore box: separationB against separationA + 0.1 linearSlop
            if st.kind == 1:
                for body in bodies()[:5]:
                    for phi in (0.05, 0.3, -0.2):
                        got = _flip_boundary(st, body, phi)
                        if got is None:
                            continue
                        for ctl, shift in (("#", 0.0), ("~", 0.02)):       # (the control stands 2 cm off)
                            cx, cy, ang = got
                            T.ladder("bb/flip%s%d%s" % (ctl, lid, tag), st, body, np.array([cx + shift, cy]), np.array([1.0, 0.0]), ang)
                        lid += 1
    _exact_cases(T)
    return T.done()


def flip_ties():
    """Box-on-hardcore-box cases where b2CollidePolygons' separationB == separationA + 0.1 b2_linearSlop TO THE BIT (the flip
    rule's `>` keeps the hardcore box's face there, a `>=` would not): found once by scanning binary32 neighbours of the flip
    boundaries with rem2d_oracle_kat_polygon_separations, kept as tests/golden/geometry_flip_ties.npy, float32 [19, 18]; the host
    half re-checks the equality."""
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry_flip_ties.npy"))


def _exact_cases(T):
    """Boundaries met to the bit, on geometry where binary32 can: an edge through y = 0 (so a centre `radius` above an end point
    has d = (0, radius) exactly and dd == rr), each with its neighbours one ulp either side in y."""
    for off in OFFSETS:
        x0 = float(f32(off + 3 * PITCH))
        st = Static(0, [x0, 0.0, float(f32(x0 + PITCH)), 0.0], "edge_y0")
        for r in CIRCLES:
            radius = f32(f32(0.01) + f32(r))         # b2_polygonRadius + the circle's, as the routine forms it
            for end in (0, 2):
                for y in ladder(radius, 1):
                    T.add("ec/dd_eq_rr@%g" % off, st, (2, r, 0.0), (float(st.raw[end]), y), 0.0)
                for y in ladder(-float(radius), 1):
                    T.add("ec/dd_eq_rr@%g" % off, st, (2, r, 0.0), (float(st.raw[end]), y), 0.0)


def _separations(st, body, c, ang):
    """b2FindMaxSeparation both ways in binary64 for an axis-aligned hardcore box and a module box."""
    xs, ys = st.raw[0::2].astype(f64), st.raw[1::2].astype(f64)
    A = np.array([[xs.min(), ys.min()], [xs.max(), ys.min()], [xs.max(), ys.max()], [xs.min(), ys.max()]])
    nA = np.array([[0, -1.0], [1.0, 0], [0, 1.0], [-1.0, 0]])
    hx, hy = body[1], body[2]
    R = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    B = (R @ np.array([[-hx, -hy], [hx, -hy], [hx, hy], [-hx, hy]]).T).T + np.asarray(c)
    nB = (R @ nA.T).T
    sA = max(min(float(nA[i] @ (B[j] - A[i])) for j in range(4)) for i in range(4))
    sB = max(min(float(nB[i] @ (A[j] - B[i])) for j in range(4)) for i in range(4))
    return sA, sB


def _flip_boundary(st, body, phi):
    """A tilted box sliding off the top face's right end: the x (binary64) at which separationB - separationA crosses 0.1
    linearSlop, by bisection; None where it does not cross."""
    a, b = st.frames[0]
    y = a[1] + extent(body, phi) + 0.25 * POLY_R

    def g(x):
        sA, sB = _separations(st, body, (x, y), phi)
        return (sB - sA) - 0.1 * SLOP
    lo, hi = b[0] - 0.05, b[0] + body[1] + body[2] + 0.05
    xs = np.linspace(lo, hi, 400)
    gs = np.array([g(x) for x in xs])
    idx = [i for i in np.nonzero((gs[:-1] <= 0) != (gs[1:] <= 0))[0]          # (a crossing where the boxes touch: both
           if max(_separations(st, body, (xs[i], y), phi)) < 0.75 * 2 * POLY_R]  # separations inside the contact radius)
    if len(idx) == 0:
        return None
    lo, hi = xs[idx[0]], xs[idx[0] + 1]
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if (g(mid) <= 0) == (g(lo) <= 0):
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi), y, phi


# ---- distance --------------------------------------------------------------------------------------------------------------
def distance_cases():
    T = Table()
    for off in OFFSETS:
        tag = "@%g" % off
        for st in statics(off):
            for body in bodies():
                box = body[0] == 1
                for fr in st.frames:
                    e, u, ang = frame(*fr)
                    # a vertex exactly on the other shape's line (distance 0) and one ulp either side
                    phi = np.arctan2(body[2], body[1]) if box else 0.0
                    for k in (-1, 0, 1):
                        T.place("vertex_on_line" + tag, st, fr, body, 0.5, 0.0, phi, dy_ulps=k)
                        T.place("vertex_on_line" + tag, st, fr, body, 1.0, 0.0, phi, dy_ulps=k)
                    # overlapping cores
                    for sep in (-0.3, -0.05, -1e-4):
                        for phi2 in (0.0, 0.5):
                            T.place("overlap" + tag, st, fr, body, 0.4, sep, phi2)
                    # parallel faces: the closest feature is not unique
                    for s in (0.0, 0.5, 1.0, 1.4):
                        for sep in (1e-4, 0.02, 0.7):
                            T.place("parallel" + tag, st, fr, body, s, sep, 0.0)
                            T.place("parallel" + tag, st, fr, body, s, sep, np.pi / 2)
                    # collinear three-point simplices: the body on the face's own line beyond its ends
                    for s in (-1.0, -0.2, 1.2, 2.0):
                        T.place("collinear" + tag, st, fr, body, s, -extent(body, 0.0), 0.0)
                        if box:   # ... and a face of the box in line with it
                            c = fr[0] + s * (fr[1] - fr[0]) - body[2] * u
                            T.add("collinear" + tag, st, body, c, ang)
                    # a point beyond an end
                    for s in (-0.5, 1.5):
                        for sep in (0.0, 0.3):
                            for phi2 in (0.0, 0.7):
                                T.place("beyond" + tag, st, fr, body, s, sep, phi2)
    spec, fam = T.done()
    bs, bf = bulk("distance", 100000, seed=11)
    return np.concatenate((spec, bs)), np.concatenate((fam, bf))


# ---- time of impact --------------------------------------------------------------------------------------------------------
TURN = 2 * np.pi


def toi_cases(with_bulk=True):
    T = Table()
    for off in OFFSETS:
        tag = "@%g" % off
        sts = statics(off)
        for si, st in enumerate(sts):
            for body in bodies():
                target = toi_target(body)
                for fr in st.frames:
                    a, b = fr
                    e, u, ang = frame(a, b)
                    L = np.hypot(*(b - a))
                    ext0 = extent(body, 0.0)

                    def at(s, h, fr=fr, u=u):
                        return fr[0] + s * (fr[1] - fr[0]) + h * u
                    # a straight drop onto the face; up to 2 m straight through it (tunnelling is stopped)
                    for s in (0.1, 0.5, 0.9):
                        T.add("drop" + tag, st, body, at(s, ext0 + 0.6), ang, at(s, ext0 - 0.1), ang)
                        T.add("through" + tag, st, body, at(s, ext0 + 0.9), ang + 0.2, at(s, ext0 - 1.1), ang + 0.2)
                        T.add("through" + tag, st, body, at(s, 1.0) - 0.5 * e, ang, at(s, -0.9) + 0.5 * e, ang + 1.0)
                    # a slide parallel to the face at clearances across target +- tolerance
                    for d in (-3, -1.5, -1.01, -0.99, -0.5, 0.0, 0.5, 0.99, 1.01, 1.5, 3, 8):
                        h = ext0 + target + d * TOL
                        T.add("slide" + tag, st, body, at(-1.5 / L, h), ang, at(1.0 + 0.4 / L, h), ang)
                        T.add("slide" + tag, st, body, at(0.1, h), ang, at(0.9, h), ang)
                    # pure rotations up to +-pi/2 (b2_maxRotation) at heights the corners sweep through
                    R = np.hypot(body[1], body[2]) if body[0] == 1 else 0.0
                    for da in (np.pi / 2, -np.pi / 2, np.pi / 4, -0.1):
                        for h in (ext0 + target + 3 * TOL, 0.5 * (ext0 + R) + target, R + target - TOL, R + target + 3 * TOL):
                            T.add("rotate" + tag, st, body, at(0.5, h), ang, at(0.5, h), ang + da)
                            T.add("rotate" + tag, st, body, at(1.0, h), ang, at(1.0, h), ang + da)
                    # across an end point / over the vertex two edges share (the neighbour sees the same sweep below)
                    for h in (ext0 + target - TOL, ext0 + target + 2 * TOL, ext0 + 0.05):
                        T.add("end" + tag, st, body, at(1.0 + 0.8 / L, h - 0.3), ang - 0.4, at(1.0 - 0.3 / L, h), ang + 0.3)
                        T.add("end" + tag, st, body, at(-0.9 / L, h + 0.2), ang, at(0.2, h), ang)
                        T.add("end" + tag, st, body, at(1.0, h + 0.5), ang, at(1.0, h - 0.6), ang)
                    # touching at the start, overlapped at the start
                    for dh in (-TOL, 0.0, 0.9 * TOL):
                        T.add("touching0" + tag, st, body, at(0.5, ext0 + target + dh), ang, at(0.6, ext0 + 0.5), ang + 0.3)
                    for dh in (-1e-4, -0.02, -0.3):
                        T.add("overlapped0" + tag, st, body, at(0.5, ext0 + dh), ang, at(0.6, ext0 + 0.5), ang + 0.3)
                    # a0 at 40 and -1000 turns: b2Sweep::Normalize
                    for turns in (40.0, -1000.0):
                        a0 = float(f32(ang + 0.2 + turns * TURN))
                        for da in (0.0, 1.2, -np.pi / 2):
                            T.add("turns" + tag, st, body, at(0.5, R + 0.5), a0, at(0.5, ext0 - 0.2), a0 + da)
            # the vertex shared with the next edge: the same sweeps seen from both edges
            if st.kind == 0 and si + 1 < len(sts) and sts[si + 1].kind == 0 and st.name != "riser":
                a, b = st.frames[0]
                nxt = Static(0, [b[0], b[1], b[0] + PITCH, b[1] - 0.3 * PITCH], st.name + "+next")
                for body in bodies():
                    ext0 = extent(body, 0.0)
                    for dx in (-0.05, 0.0, 0.05):
                        c0, c = (b[0] + dx, b[1] + ext0 + 0.8), (b[0] + dx + 0.1, b[1] + ext0 - 0.4)
                        for s2 in (st, nxt):
                            T.add("shared_vertex" + tag, s2, body, c0, 0.1, c, 0.9)
    _many_turns(T, 6000, seed=13)
    spec, fam = T.done()
    if with_bulk:
        bs, bf = bulk("toi", 30000, seed=12)
        spec, fam = np.concatenate((spec, bs)), np.concatenate((fam, bf))
    return spec, fam


def _many_turns(T, n, seed):
    """Sweeps no step produces (the engine clamps a step to 2 m and pi / 2): grazing passes of up to some metres while the body
    turns by up to +-60 rad.  The separation along the sweep oscillates, and these are the cases in which b2TimeOfImpact's root
    finder needs more than a handful of its 50 iterations (a finder capped at 10 answers about one in twenty of them
    differently); the routines must agree on any finite input."""
    rng = np.random.RandomState(seed)
    pool = {off: statics(off) for off in OFFSETS}
    bod = bodies()
    for i in range(n):
        off = OFFSETS[i & 1]
        st = pool[off][rng.randint(len(pool[off]))]
        body = bod[rng.randint(len(bod))]
        fr = st.frames[rng.randint(len(st.frames))]
        e, u, ang = frame(*fr)
        R = np.hypot(body[1], body[2]) if body[0] == 1 else body[1]
        c0 = fr[0] + rng.uniform(-3, 0) * (fr[1] - fr[0]) + R * rng.uniform(0.2, 1.6) * u
        c1 = fr[0] + rng.uniform(1, 4) * (fr[1] - fr[0]) + R * rng.uniform(0.2, 1.6) * u
        a0 = ang + rng.uniform(-np.pi, np.pi)
        T.add("many_turns@%g" % off, st, body, c0, a0, c1, a0 + rng.uniform(-60, 60))


# ---- bulk: random pairs within [-0.1, +0.05] m of contact ---------------------------------------------------------------------
def bulk(op, n, seed):
    rng = np.random.RandomState(seed)
    T = Table()
    pool = {off: statics(off) for off in OFFSETS}
    bod = bodies()
    for i in range(n):
        off = OFFSETS[i & 1]
        st = pool[off][rng.randint(len(pool[off]))]
        body = bod[rng.randint(len(bod))]
        fr = st.frames[rng.randint(len(st.frames))]
        e, u, ang = frame(*fr)
        s, phi = rng.uniform(-0.4, 1.4), rng.uniform(-np.pi, np.pi)
        rad = POLY_R + (POLY_R if body[0] == 1 else body[1])
        gap = rad + rng.uniform(-0.1, 0.05)                              # of the core shapes
        c = fr[0] + s * (fr[1] - fr[0]) + (extent(body, phi) + gap) * u
        if op == "toi":     # a sweep that ends there, from up to 2 m and pi / 2 away
            d = rng.uniform(0.0, 2.0) * np.array([np.cos(rng.uniform(0, 2 * np.pi)), 1.0])
            d = d / max(1.0, np.hypot(*d) / 2.0)
            back = rng.uniform(0.3, 1.5)
            c0 = c + back * (d[0] * e + abs(d[1]) * u)
            c1 = c - (1.0 - min(back, 1.0)) * 0.3 * u
            T.add("bulk@%g" % off, st, body, c0, ang + phi + rng.uniform(-np.pi / 2, np.pi / 2) * rng.randint(2), c1, ang + phi)
        else:
            T.add("bulk@%g" % off, st, body, c, ang + phi)
    return T.done()


def collide_bulk(n=60000, seed=10):
    """... and the exact flip ties, as family 'bb/flip_tie'."""
    spec, fam = bulk("collide", n, seed)
    ties = flip_ties()
    return np.concatenate((spec, ties)), np.concatenate((fam, np.array(["bb/flip_tie"] * len(ties))))


# ---- the near-miss family of the exact skip -----------------------------------------------------------------------------------
NEAR_PASSES = ("edge", "end", "corner")
NEAR_MOTIONS = ("translate", "turn", "both")
# clearance - need, 48 per sub-family, 20 (circles) / 28 (boxes) of them below need.  A box's need is 6.25 mm: below need - 6.25 mm its core crosses the
# static core and b2TimeOfImpact answers "overlapped" (alpha = 1), so all but four of a box's 28 keep the cores apart
NEAR_CLEAR = {"circle": np.concatenate((np.linspace(-0.02, -0.0005, 20), np.linspace(0.0005, 0.05, 28))),
              "box": np.concatenate((np.linspace(-0.02, -0.008, 4), np.linspace(-0.0056, -0.0008, 24), np.linspace(0.0005, 0.05, 20)))}


def _pt_seg(p, a, b):
    ab = b - a
    den = (ab * ab).sum(-1)
    t = np.clip(((p - a) * ab).sum(-1) / np.where(den > 0, den, 1.0), 0.0, 1.0)
    d = p - (a + t[..., None] * ab)
    return np.sqrt((d * d).sum(-1))


def closest_approach(st, body, c0, c1, a0, da, samples=257):
    """Smallest distance of the core shapes over the sweep, binary64, sampled (vertex-to-segment distances both ways: valid
    while the cores stay apart)."""
    r = st.raw.astype(f64)
    if st.kind == 0:
        A = np.array([r[0:2], r[2:4]])
        segA = (A[:1], A[1:])
    else:
        xs, ys = r[0::2], r[1::2]
        A = np.array([(xs.min(), ys.min()), (xs.max(), ys.min()), (xs.max(), ys.max()), (xs.min(), ys.max())])
        segA = (A, np.roll(A, -1, axis=0))
    t = np.linspace(0.0, 1.0, samples)
    c = np.asarray(c0, f64) + t[:, None] * (np.asarray(c1, f64) - np.asarray(c0, f64))
    if body[0] == 2:
        B = c[:, None, :]
        segB = (B, B)
    else:
        ang = a0 + t * da
        loc = np.array([(-body[1], -body[2]), (body[1], -body[2]), (body[1], body[2]), (-body[1], body[2])])
        cs, sn = np.cos(ang)[:, None], np.sin(ang)[:, None]
        B = np.stack((cs * loc[:, 0] - sn * loc[:, 1], sn * loc[:, 0] + cs * loc[:, 1]), -1) + c[:, None, :]
        segB = (B, np.roll(B, -1, axis=1))
    d1 = _pt_seg(B[:, :, None, :], segA[0][None, None], segA[1][None, None]).min()
    d2 = _pt_seg(A[None, :, None, :], segB[0][:, None], segB[1][:, None]).min()
    return float(min(d1, d2))


def near_miss_cases():
    """(spec, family): family = 'near/<pass>/<motion>/<box|circle>@<offset>', 48 clearances each (NEAR_CLEAR): the body passes
    the middle of an edge, an edge's end, or a hardcore box's corner, translating up to 2 m, turning by up to pi / 2, or both.
    The clearance is the smallest core distance over the sweep (sampled in binary64 at need + 0.05 and lowered from there)."""
    T = Table()
    boxes, circs = bodies()[:5], bodies()[5:]
    for off in OFFSETS:
        sts = statics(off)
        eds, hbs = [s for s in sts if s.kind == 0], [s for s in sts if s.kind == 1]
        for pas in NEAR_PASSES:
            for mot in NEAR_MOTIONS:
                for kind, blist in (("box", boxes), ("circle", circs)):
                    fam = "near/%s/%s/%s@%g" % (pas, mot, kind, off)
                    for j, dclear in enumerate(NEAR_CLEAR[kind]):
                        body = blist[j % len(blist)]
                        st = (hbs if pas == "corner" else eds)[j % (len(hbs) if pas == "corner" else len(eds))]
                        a, b = st.frames[0]
                        e, u, ang = frame(a, b)
                        L = np.hypot(*(b - a))
                        mid = {"edge": a + 0.5 * (b - a), "end": b + 0.0 * e, "corner": b}[pas]
                        da = (0.1, 0.3, 0.8, np.pi / 2)[j % 4] * (1 if j % 8 < 4 else -1) if mot != "translate" else 0.0
                        span = (0.3, 0.8, 1.4, 2.0)[(j // 4) % 4] if mot != "turn" else 0.0
                        a0 = ang + (0.0 if mot == "translate" else -0.5 * da + (0.4 if j % 3 == 0 else 0.0))
                        R = np.hypot(body[1], body[2]) if body[0] == 1 else 0.0
                        # past an end / a corner the body goes by beside it, on the line of the face: start out in the open
                        if pas == "edge":
                            base, along, out = mid, e, u
                        else:
                            base, along, out = mid, u, e
                        hgt = R + 0.3

                        def sweep(h):
                            c0 = base - 0.5 * span * along + h * out
                            c1 = base + 0.5 * span * along + h * out
                            if mot == "turn":      # a point's turn is no motion at all: give the circle's centre 1 cm of travel
                                c0, c1 = base + h * out - 0.005 * along, base + h * out + 0.005 * along
                            return c0, c1

                        def closest(h):
                            c0, c1 = sweep(h)
                            return closest_approach(st, body, c0, c1, a0, da)
                        want = need_of(body) + 0.05
                        for _ in range(4):
                            hgt += want - closest(hgt)
                        hgt -= 0.05 - dclear
                        if need_of(body) + dclear > 1e-3:       # the cores stay apart: the clearance itself can be met
                            for _ in range(3):
                                hgt += need_of(body) + dclear - closest(hgt)
                        c0, c1 = sweep(hgt)
                        T.add(fam, st, body, c0, a0, c1, a0 + da)
    return T.done()


# ---- the device's table ---------------------------------------------------------------------------------------------------------
def library_static_box(lib):
    """static_box for device_table from a loaded librem2d (ctypes): rem2d_selftest_static_box."""
    def static_box(xy):
        out = np.zeros(16, f32)
        rc = lib.rem2d_selftest_static_box(xy.ctypes.data, out.ctypes.data)
        assert rc == 0, lib.rem2d_last_error()
        return out
    return static_box


def device_table(spec, static_box):
    """The oracle's table -> the device's (include/rem2d_selftest.h).  static_box(xy float32 [8]) -> float32 [16]: the library's
    rem2d_selftest_static_box, i.e. the terrain upload's own derivation of a hardcore box's vertices and normals."""
    n = len(spec)
    dev = np.zeros((n, DEVICE_WORDS), f32)
    dev[:, 0] = spec[:, 0]
    edge = spec[:, 0] == 0
    dev[edge, 1:5] = spec[edge, 1:5]
    cache = {}
    for i in np.nonzero(~edge)[0]:
        key = spec[i, 1:9].tobytes()
        if key not in cache:
            cache[key] = np.asarray(static_box(np.ascontiguousarray(spec[i, 1:9])), f32)
        dev[i, 1:17] = cache[key]
    dev[:, 17:26] = spec[:, 9:18]
    return dev


if __name__ == "__main__":
    for name, fn in (("collide", collide_cases), ("collide bulk", collide_bulk), ("distance", distance_cases), ("toi", toi_cases),
                     ("near miss", near_miss_cases)):
        spec, fam = fn()
        print("%-14s %7d cases in %d families" % (name, len(spec), len(set(fam))))
