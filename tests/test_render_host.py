"""The renderer without a GPU: the numpy pixel model (tests/render_model.py) against pixel sets computed by hand in float64,
the reference's scrolling camera, and the library's exports of include/rem2d_render.h."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import render_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 120, 90
PX = 1.0 / 30.0


def centres(cam, width=W, height=H):
    """float64 pixel centres (X [H, W], Y [H, W]) of the spec's formula."""
    i, j = np.arange(width) + 0.5, np.arange(height) + 0.5
    X = cam[0] + i * PX
    Y = cam[1] + height * PX - j * PX
    return np.meshgrid(X, Y)


def colour_mask(img, rgb):
    return np.all(img == np.array(rgb, np.uint8), axis=-1)


def check_sets(img, sure_in, sure_line, sure_out, fill, line, back):
    """Every pixel the float64 geometry classifies with a margin gets the colour of its class."""
    assert sure_in.sum() > 20 and sure_line.sum() > 20 and sure_out.sum() > 20
    assert colour_mask(img, fill)[sure_in].all()
    assert colour_mask(img, line)[sure_line].all()
    assert colour_mask(img, back)[sure_out].all()


def box_sets(X, Y, cx, cy, hx, hy, ang, eps=0.02 * PX):
    """(inside, on the 2-px outline, outside) of a box, each with a margin of eps to every boundary (float64)."""
    c, s = math.cos(ang), math.sin(ang)
    u = c * (X - cx) + s * (Y - cy)   # box frame
    v = -s * (X - cx) + c * (Y - cy)
    du, dv = np.abs(u) - hx, np.abs(v) - hy
    # distance to the outline band's axes: within the band if within PX of an edge line and within that edge's extent
    near_u = (np.abs(du) < PX - eps) & (np.abs(v) < hy - eps)
    near_v = (np.abs(dv) < PX - eps) & (np.abs(u) < hx - eps)
    far_u = (np.abs(du) > PX + eps) | (np.abs(v) > hy + eps)
    far_v = (np.abs(dv) > PX + eps) | (np.abs(u) > hx + eps)
    band = near_u | near_v
    no_band = far_u & far_v
    inside = (du < -eps) & (dv < -eps) & no_band
    outside = ((du > eps) | (dv > eps)) & no_band
    return inside, band, outside


@pytest.fixture(scope="module")
def sincosf():
    from oracle import oracle as O
    O.build()
    return O.sincosf


def test_axis_aligned_box(sincosf):
    cam = (10.0, 3.0)
    cx, cy, hx, hy = 11.5, 4.2, 0.6, 0.35
    img = M.render(W, H, cam, bodies=[(1, cx, cy, 0.0, hx, hy)], sincosf=sincosf)
    X, Y = centres(cam)
    check_sets(img, *box_sets(X, Y, cx, cy, hx, hy, 0.0), M.BOX_FILL, M.BOX_LINE, M.SKY)
    # hand count: the fill spans the pixel columns whose centres lie in (cx - hx + 1 px, cx + hx - 1 px)
    row = img[int((cam[1] + H * PX - cy) / PX)]
    cols = np.nonzero(colour_mask(row[None], M.BOX_FILL)[0])[0]
    assert len(cols) == round(2 * (hx - PX) / PX)


def test_rotated_box(sincosf):
    cam = (20.0, 0.0)
    cx, cy, hx, hy, ang = 22.0, 1.5, 0.8, 0.3, 0.7
    img = M.render(W, H, cam, bodies=[(1, cx, cy, ang, hx, hy)], sincosf=sincosf)
    X, Y = centres(cam)
    check_sets(img, *box_sets(X, Y, cx, cy, hx, hy, ang), M.BOX_FILL, M.BOX_LINE, M.SKY)


def test_disc_with_ring(sincosf):
    cam = (30.0, 2.0)
    cx, cy, r = 31.9, 3.4, 0.5
    img = M.render(W, H, cam, bodies=[(2, cx, cy, 1.234, r, 0.0)], sincosf=sincosf)
    X, Y = centres(cam)
    d = np.hypot(X - cx, Y - cy)
    e = 0.02 * PX
    check_sets(img, d < r - PX - e, (d > r - PX + e) & (d < r + PX - e), d > r + PX + e, M.CIRCLE_FILL, M.CIRCLE_LINE, M.SKY)


def sloped_terrain():
    # four edges of pitch 1, the second one sloped from y = 1 to y = 2
    return M.Terrain([40.0, 41.0, 42.0, 43.0, 44.0], [1.0, 1.0, 2.0, 2.0, 2.0])


def test_ground_under_a_sloped_edge(sincosf):
    cam = (40.0, 0.0)
    img = M.render(W, H, cam, terrain=sloped_terrain(), sincosf=sincosf)
    X, Y = centres(cam)
    sel = (X > 41.0 + 2 * PX) & (X < 42.0 - 2 * PX)   # under edge 1 only
    line_y = 1.0 + (X - 41.0)
    dist = (Y - line_y) / math.sqrt(2.0)               # signed distance to the edge
    e = 0.02 * PX
    below = sel & (dist < -PX - e) & (Y > e)
    above = sel & (dist > PX + e)
    on = sel & (np.abs(dist) < PX - e)
    assert colour_mask(img, M.GROUND)[below].all() and below.sum() > 100
    assert colour_mask(img, M.SKY)[above].all() and above.sum() > 100
    assert colour_mask(img, M.EDGE_ODD)[on].all() and on.sum() > 20       # edge 1 is odd
    flat0 = (X > 40.0 + 2 * PX) & (X < 41.0 - 2 * PX) & (np.abs(Y - 1.0) < PX - e)
    assert colour_mask(img, M.EDGE_EVEN)[flat0].all() and flat0.sum() > 20
    # below y = 0 there is no ground
    img2 = M.render(W, H, (40.0, -2.0), terrain=sloped_terrain(), sincosf=sincosf)
    X2, Y2 = centres((40.0, -2.0))
    assert colour_mask(img2, M.SKY)[(Y2 < -e) & (X2 > 40.5) & (X2 < 43.5)].all()


def test_painter_order_body_over_ground(sincosf):
    cam = (40.0, 0.0)
    t = sloped_terrain()
    cx, cy, hx, hy = 43.0, 1.0, 0.5, 0.4    # sunk into the ground under the flat edges
    fill, line = [(200, 10, 10)], [(10, 10, 200)]
    img = M.render(W, H, cam, terrain=t, bodies=[(1, cx, cy, 0.0, hx, hy)], fill=fill, line=line, sincosf=sincosf)
    X, Y = centres(cam)
    inside, band, outside = box_sets(X, Y, cx, cy, hx, hy, 0.0)
    assert colour_mask(img, fill[0])[inside].all()
    assert colour_mask(img, line[0])[band].all()
    ground = outside & (Y < 2.0 - 2 * PX) & (Y > 0.01) & (X > 42.0 + 2 * PX)
    assert colour_mask(img, M.GROUND)[ground].all() and ground.sum() > 100
    # a second body in a later slot covers the first
    img2 = M.render(W, H, cam, terrain=t, bodies=[(1, cx, cy, 0.0, hx, hy), (2, cx, cy, 0.0, 0.2, 0.0)], sincosf=sincosf,
                    fill=fill + [(1, 2, 3)], line=line + [(4, 5, 6)])
    d = np.hypot(X - cx, Y - cy)
    assert colour_mask(img2, (1, 2, 3))[d < 0.2 - 1.1 * PX].all()


def test_camera_at_negative_coordinates(sincosf):
    cam = (-12.0, -7.5)
    cx, cy, hx, hy = -10.8, -6.1, 0.4, 0.5
    img = M.render(W, H, cam, bodies=[(1, cx, cy, 0.0, hx, hy)], wod=-11.51, sincosf=sincosf)
    X, Y = centres(cam)
    inside, band, outside = box_sets(X, Y, cx, cy, hx, hy, 0.0)
    check_sets(img, inside, band, outside & (np.abs(X + 11.51) > PX), M.BOX_FILL, M.BOX_LINE, M.SKY)
    # the wall of death: one pixel column, from y = -10 up
    col = np.nonzero(colour_mask(img, M.WOD).any(axis=0))[0]
    assert len(col) == 1 and abs(X[0, col[0]] + 11.51) <= 0.5 * PX
    rows = np.nonzero(colour_mask(img, M.WOD)[:, col[0]])[0]
    assert Y[rows, col[0]].min() >= -10.0 and len(rows) == H   # (the whole view is above y = -10 + ...)


def test_flag_and_wall_of_death_limits(sincosf):
    cam = (0.0, 4.0)
    img = M.render(W, H, cam, wod=0.5, sincosf=sincosf)
    X, Y = centres(cam)
    tri = (X > M.FLAG_X + 3 * PX) & (X < M.FLAG_X + 0.3) & (np.abs(Y - 6.5) < 0.03)
    assert colour_mask(img, M.FLAG_FILL)[tri].all() and tri.sum() > 5
    pole = (np.abs(X - 1.4) < 0.5 * PX) & (Y > 5.0 + 2 * PX) & (Y < 6.3)
    assert colour_mask(img, M.FLAG_LINE)[pole].all() and pole.sum() > 10
    img2 = M.render(W, H, (0.0, 39.0), wod=0.5, sincosf=sincosf)
    _, Y2 = centres((0.0, 39.0))
    c = colour_mask(img2, M.WOD).any(axis=1)
    assert c[Y2[:, 0] <= 40.0 - 0.01].all() and not c[Y2[:, 0] > 40.0].any()


def test_reference_camera_reproduces_the_scroll():
    """render.ReferenceCamera == the reference's step() arithmetic (Modular2DEnv.py:636-641), in Python floats, on a recorded
    root trajectory (float32 positions, as pybox2d hands them out)."""
    import torch
    from gym_rem2d_amd.render import ReferenceCamera
    rng = np.random.default_rng(3)
    traj = np.cumsum(rng.normal(0.02, 0.05, size=(200, 2)), axis=0).astype(np.float32) + np.float32([5.0, 7.0])
    cam = ReferenceCamera(1, device="cpu")
    scroll = scroll_y = prevscroll = prevscroll_y = 0.0
    assert cam.xy.tolist() == [[0.0, 0.0]]   # reset()
    for x, y in traj:
        x, y = float(x), float(y)
        x_scroll = x - 800 / 30.0 / 5
        y_scroll = y - 600 / 30.0 / 4
        scroll = x_scroll + 0.99 * (x_scroll - prevscroll)
        scroll_y = y_scroll + 0.99 * (y_scroll - prevscroll_y)
        prevscroll, prevscroll_y = x_scroll, y_scroll
        cam.update(torch.tensor([x], dtype=torch.float64), torch.tensor([y], dtype=torch.float64))
        assert cam.scroll.item() == scroll and cam.scroll_y.item() == scroll_y
        assert cam.xy[0].tolist() == [float(np.float32(scroll)), float(np.float32(scroll_y))]


def test_library_exports_the_render_header():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    with open(os.path.join(ROOT, "include", "rem2d_render.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*int\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert set(declared) == {"rem2d_world_render", "rem2d_render_abi_version"}
    assert int(re.search(r"#define REM2D_RENDER_ABI_VERSION (\d+)", text).group(1)) == _lib.RENDER_ABI_VERSION
    assert int(re.search(r"#define REM2D_RENDER_MAX_SIZE (\d+)", text).group(1)) == _lib.RENDER_MAX_SIZE
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in declared:
            assert (" T " + name) in syms, (path, name)


def test_palette_matches_the_reference_colours():
    from gym_rem2d_amd import render as R
    assert R.SKY == R.to_uint8((0.9, 0.9, 1.0)) == M.SKY
    assert R.GROUND == R.to_uint8((0.4, 0.6, 0.3)) == M.GROUND
    assert R.EDGE_EVEN == R.to_uint8((0.3, 1.0, 0.3)) and R.EDGE_ODD == R.to_uint8((0.3, 0.8, 0.3))
    assert R.OBSTACLE_LINE == R.to_uint8((0.6, 0.6, 0.6)) and R.FLAG_FILL == R.to_uint8((0.9, 0.2, 0))
    # and the kernel's constants say the same
    with open(os.path.join(ROOT, "gym_rem2d_amd", "csrc", "rem2d_raster.h")) as f:
        text = f.read()
    for name, rgb in (("SKY", R.SKY), ("GROUND", R.GROUND), ("EDGE_EVEN", R.EDGE_EVEN), ("EDGE_ODD", R.EDGE_ODD),
                      ("OBST_FILL", R.OBSTACLE_FILL), ("OBST_LINE", R.OBSTACLE_LINE), ("WOD", R.WALL_OF_DEATH),
                      ("FLAG_LINE", R.FLAG_LINE), ("FLAG_FILL", R.FLAG_FILL), ("BOX_FILL", R.BOX_FILL), ("BOX_LINE", R.BOX_LINE),
                      ("CIRCLE_FILL", R.CIRCLE_FILL), ("CIRCLE_LINE", R.CIRCLE_LINE)):
        m = re.search(r"RC_%s = RGB\((\d+), (\d+), (\d+)\)" % name, text)
        assert m and tuple(int(v) for v in m.groups()) == rgb, name


def test_tree_colors_follow_viridis():
    """Default body colours of a tree: viridis(node.type / len(module_list)), fill == outline (simple_module.py:299-304)."""
    import copy
    import random
    from gym_rem2d_amd import get_module_list, render as R
    from gym_rem2d_amd.compiler import build_creature
    from gym_rem2d_amd.encodings import DirectEncoding
    random.seed(5)
    ml = get_module_list()
    g = DirectEncoding(ml)
    tree = copy.deepcopy(g.create(4))
    _, comps, _ = build_creature(tree.getNodes(), ml)
    fill, line = R.tree_colors(tree, ml, 64)
    import matplotlib
    cmap = matplotlib.colormaps["viridis"]
    seen = 0
    for node in tree.getNodes():
        if node.expressed and node.component:
            want = tuple(int(round(255 * c)) for c in cmap(node.type / len(ml))[:3])
            assert tuple(fill[node.component[0].slot]) == want == tuple(line[node.component[0].slot])
            seen += 1
    assert seen == len(comps) >= 1
