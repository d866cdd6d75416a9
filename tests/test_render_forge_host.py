"""The forged render scenes without a GPU (tests/render_forge.py): the brute mode of the pixel model against its windowed mode over
every terrain of terrain_forge, and the conditions that keep the GPU half (tests/test_render_forge_gpu.py) from being vacuous --
the per-tile obstacle counts that give the obstacle scenes their names, a painter order that shows, knife-edge pixels that a
contracted evaluation of the edge functions really changes, and in every scene pixels of each colour class it is there for."""
import numpy as np
import pytest

import render_forge as RF
import render_model as M
import terrain_forge as TF

f32 = np.float32
PX = RF.PX


@pytest.fixture(scope="module")
def sincosf():
    from oracle import oracle as O
    O.build()
    return O.sincosf


_FRAMES = {}


def frames(name, sincosf):
    if name not in _FRAMES:
        s = RF.scenes()[name]
        _FRAMES[name] = RF.model_frames(s, s.state(), sincosf)
    return _FRAMES[name]


def has(img, rgb, at_least=1):
    return int(RF.colour_mask(img, rgb).sum()) >= at_least


def test_scene_list():
    assert list(RF.scenes()) == RF.names() and len(set(RF.names())) == len(RF.names())


# --------------------------------------------------------------------------------------------------------- brute == windowed
@pytest.mark.parametrize("name", list(TF.TERRAINS))
def test_brute_model_equals_windowed(name, sincosf):
    """240 x 150 views tiling the whole track along the ground, one wholly left of xs[0], one wholly right of xs[-1] and one
    below y = 0: the +-1 edge window of the windowed mode (the kernel's) loses and adds no pixel.  Pitches under 2 px are not
    chased: a line is 2 px wide, the window cannot cover them, and no track has them."""
    prof = TF.profile(name)
    T = M.Terrain.of(prof)
    xs, ys = np.asarray(prof.xs), np.asarray(prof.ys)
    w, h = 240, 150
    vw, vh = w * PX, h * PX
    cams = []
    x = xs[0] - 0.5 * vw
    while x < xs[-1]:
        inside = (xs >= x) & (xs <= x + vw)
        mid = 0.5 * (ys[inside].min() + ys[inside].max()) if inside.any() else ys[np.argmin(np.abs(xs - x))]
        cams.append((x, mid - 0.5 * vh))
        x += vw
    cams += [(xs[0] - vw - 0.05, ys[0] - 0.5 * vh), (xs[-1] + 0.05, ys[-1] - 0.5 * vh), (xs[len(xs) // 3], -vh - 0.01)]
    ground = lines = 0
    for cam in cams:
        a = M.render(w, h, cam, terrain=T, flag=False, sincosf=sincosf, brute=True)
        b = M.render(w, h, cam, terrain=T, flag=False, sincosf=sincosf)
        assert np.array_equal(a, b), "%s, view at %s: %d pixels differ" % (name, cam, int(np.any(a != b, axis=-1).sum()))
        ground += int(RF.colour_mask(a, M.GROUND).sum())
        lines += int((RF.colour_mask(a, M.EDGE_EVEN) | RF.colour_mask(a, M.EDGE_ODD)).sum())
    for k, cam in enumerate(cams[-3:]):       # beyond the ends there is nothing; below y = 0 no ground (hardcore4 dips under it: lines only)
        img = M.render(w, h, cam, terrain=T, flag=False, sincosf=sincosf, brute=True)
        assert not has(img, M.GROUND) and (k == 2 or not (has(img, M.EDGE_EVEN) or has(img, M.EDGE_ODD))), cam
    print("%s: %d views, %d ground and %d edge-line pixels" % (name, len(cams), ground, lines))
    assert ground > 20000 and lines > 1000


# ------------------------------------------------------------------------------------------------------------------ obstacles
def _counts(name):
    s = RF.scenes()[name]
    lists = RF.tile_lists(s.profile, RF.OBST_CAM, RF.W0, RF.H0)
    return s, lists, {k: len(v) for k, v in lists.items()}


def test_obstacle_counts_per_tile():
    """the kernel's own rule (fat AABB against the tile's pixel-centre span) gives each scene the case it is named for"""
    t = RF.OBST_TILE
    s, lists, n = _counts("obst64")
    assert len(s.profile.polys) == 64 and n[t] == 64 == max(n.values())             # the list exactly full, no overflow anywhere
    s, lists, n = _counts("obst65")
    assert len(s.profile.polys) == 65 and n[t] == 65 and sorted(n.values())[-2] <= 64
    s, lists, n = _counts("obst130")
    assert len(s.profile.polys) == 130 and max(n.values()) <= 64
    # a list fed by all three ballot passes (indices 129..66, 65..2, 1..0 in drawing order), and several fed by two
    three = [k for k, v in lists.items() if (v >= 66).any() and ((v >= 2) & (v < 66)).any() and (v < 2).any()]
    two = [k for k, v in lists.items() if (v >= 66).any() and (v < 66).any()]
    assert len(three) >= 1 and len(two) >= 8 and max(n.values()) >= 16
    s, lists, n = _counts("obst130_70")
    assert len(s.profile.polys) == 130 and n[t] == 70
    assert all(v <= 64 for k, v in n.items() if k != t)
    near = [n[t[0] + a, t[1] + b] for a in (-1, 0, 1) for b in (-1, 0, 1) if (a, b) != (0, 0)]
    assert min(near) >= 1 and sum(v > 0 for v in n.values()) >= 16                   # neighbours list fewer, most tiles some
    print({k: (n[t], max(n.values())) for k, (_, _, n) in ((m, _counts(m)) for m in ("obst64", "obst65", "obst130", "obst130_70"))})


@pytest.mark.parametrize("name", ["obst64", "obst65", "obst130", "obst130_70"])
def test_obstacle_order_is_visible(name, sincosf):
    """exchanging the indices of two overlapping boxes changes the model's frame -- inside the tile the scene is about"""
    s = RF.scenes()[name]
    base = frames(name, sincosf)[0][0]
    assert has(base, M.OBST_FILL, 200) and has(base, M.OBST_LINE, 500)
    lists = RF.tile_lists(s.profile, RF.OBST_CAM, RF.W0, RF.H0)
    t = RF.OBST_TILE if name != "obst130" else max(lists, key=lambda k: len(lists[k]))
    mine = lists[t]
    rows, cols = slice(t[0] * 16, t[0] * 16 + 16), slice(t[1] * 64, t[1] * 64 + 64)
    ref = M.render(RF.W0, RF.H0, RF.OBST_CAM, terrain=M.Terrain.of(s.profile), flag=False, sincosf=sincosf)
    q = s.profile.polys
    lo, hi = q.min(axis=1), q.max(axis=1)
    pairs = [(int(a), int(b)) for k, a in enumerate(mine) for b in mine[k + 1:]
             if (np.minimum(hi[a], hi[b]) - np.maximum(lo[a], lo[b]) > 3 * PX).all()][:8]       # bounding boxes 3 px into each other
    assert len(pairs) == 8
    changed = 0
    for a, b in pairs:
        img = M.render(RF.W0, RF.H0, RF.OBST_CAM, terrain=M.Terrain.of(RF.swapped(s.profile, a, b)), flag=False, sincosf=sincosf)
        changed += int(np.any(img != ref))
    print("%s: %d of 8 swaps of overlapping boxes change tile %s" % (name, changed, t))
    assert changed == 8


# ---------------------------------------------------------------------------------------------------------------- knife edges
def test_contraction_changes_knife_edge_pixels(sincosf, monkeypatch):
    """A condition on the INPUT: evaluated with one product of each edge function fused, the knife scene changes colour at pixels
    of every family -- so a build that contracts the renderer's arithmetic cannot pass the three-build test unseen.  The sign of a
    cross product that cancels to 0 never shows (such a pixel lies under the edge's own line band); what shows are the ties of
    the band tests: cross^2 against h^2 |d|^2 one pixel beside a 3-4-5 edge, and dot against |d|^2 at the polyline's last
    vertex.  Counted over both choices of the fused product together (each choice is printed): a given tie pixel answers to one."""
    total = dict(quad_fill=0, quad_outline=0, ground=0)
    s = RF.scenes()["knife"]
    plain = RF.model_frames(s, s.state(), sincosf)[0]
    quad_fill = [tuple(c) for c in s.fill[0][:12]] + [M.OBST_FILL]
    quad_line = [tuple(c) for c in s.line[0][:12]] + [M.OBST_LINE]
    for which in (0, 1):
        monkeypatch.setattr(M, "_edge", RF.fused_edge(which))
        fused = RF.model_frames(s, s.state(), sincosf)[0]
        monkeypatch.undo()
        diff = np.any(fused != plain, axis=-1)

        def family(colours):
            m = np.zeros(diff.shape, bool)
            for c in colours:
                m |= RF.colour_mask(plain, c) | RF.colour_mask(fused, c)
            return int((m & diff).sum())
        n = dict(all=int(diff.sum()), quad_fill=family(quad_fill), quad_outline=family(quad_line), ground=family([M.GROUND]),
                 edge_line=family([M.EDGE_EVEN, M.EDGE_ODD]))
        print("product %d fused: pixels changed %s" % (which, n))
        assert n["all"] >= 1, which
        for k in total:
            total[k] += n[k]
    assert min(total.values()) >= 1, total
    assert np.array_equal(RF.model_frames(s, s.state(), sincosf)[0], plain)


# ------------------------------------------------------------------------------------------------------- what the scenes show
@pytest.mark.parametrize("origin", list(RF.ORIGINS))
def test_body_scenes_show_what_they_are_for(origin, sincosf):
    full, mixed = RF.scenes()["full64_" + origin], RF.scenes()["mixed64_" + origin]
    img = frames("full64_" + origin, sincosf)[0][0]
    shown_fill = [has(img, full.fill[0, k]) for k in range(64)]
    shown_line = [has(img, full.line[0, k]) for k in range(64)]
    # every placed slot paints, but the box 1.5 px outside (24); of the seeded crowd (26 ..) a few may lie wholly under later ones
    unseen = [k for k in range(64) if not (shown_fill[k] or shown_line[k])]
    assert 24 in unseen and all(k >= 26 for k in unseen if k != 24) and len(unseen) <= 4, unseen
    # the 0.4-px boxes are all outline; the discs of 0.5 px and of exactly 1 px have a fill pixel only when centred on a pixel (10, 12)
    assert not shown_fill[6] and shown_line[6] and not shown_fill[8] and shown_line[8]
    assert shown_fill[10] and shown_fill[12] and shown_line[11] and shown_line[13]
    assert RF.colour_mask(img, full.fill[0, 10]).sum() == 1
    assert has(img[:, 0], full.line[0, 23]) and not has(img[:, 1:], full.line[0, 23])          # the body wholly outside the image
    assert has(img[-1], full.line[0, 25]) and not has(img[:-1], full.line[0, 25])
    for k, (rows, cols) in {17: (slice(None), 0), 18: (slice(None), -1), 19: (0, slice(None)), 20: (-1, slice(None))}.items():
        assert has(img[rows, cols], full.line[0, k]) or has(img[rows, cols], full.fill[0, k]), k   # across each border
    # tile corners: the disc on pixel (64, 16) and the box on the corner of four tiles paint in all four
    for k, (i, j) in ((15, (64, 16)), (16, (128, 32))):
        for rows, cols in ((slice(j - 8, j), slice(i - 8, i)), (slice(j - 8, j), slice(i, i + 8)), (slice(j, j + 8), slice(i - 8, i)), (slice(j, j + 8), slice(i, i + 8))):
            assert has(img[rows, cols], full.fill[0, k]) or has(img[rows, cols], full.line[0, k]), (k, rows, cols)
    assert (has(img, M.GROUND, 1000) and has(img, M.EDGE_EVEN) and has(img, M.EDGE_ODD)) and has(img, M.WOD, 50)
    if origin == "neg":        # the second view lies below y = 0: no ground at all
        below = frames("full64_neg", sincosf)[0][1]
        assert not has(below, M.GROUND) and not has(below, M.EDGE_EVEN) and has(below, full.fill[1, 0], 100)
    if origin == "far":        # a pixel step is about 500 ulps of X there
        assert 256 < float(M.INV) / float(np.spacing(f32(RF.ORIGINS["far"][1][0][0]))) < 1024
    # the non-finite slots paint nothing (the frame equals the one with those slots empty), and would paint if they were finite
    got = frames("mixed64_" + origin, sincosf)[0]
    arrays, wod = mixed.state()
    arrays["shape"][:, list(RF.NONFINITE_SLOTS)] = 0
    assert not all(np.isfinite(mixed.arrays[k]).all() for k in ("px", "py", "ang"))
    want = RF.model_frames(mixed, (arrays, wod), sincosf)[0]
    assert np.array_equal(got, want)
    for k in RF.NONFINITE_SLOTS:
        assert shown_fill[k] or shown_line[k], k
        assert not has(got[0], mixed.fill[0, k]) and not has(got[0], mixed.line[0, k]), k
    big = got[-1]              # the creature under a box larger than the image: no sky left
    assert not has(big, M.SKY) and has(big, mixed.fill[-1, 0], 10000)
    four = frames("four_" + origin, sincosf)[0][0]
    s4 = RF.scenes()["four_" + origin]
    assert has(four, s4.fill[0, 0], 100) and has(four, s4.fill[0, 2], 100) and has(four, s4.line[0, 3], 50) and not has(four, s4.fill[0, 3])


def test_shape_scenes_show_bodies_at_every_size(sincosf):
    for w, h in RF.SIZES:
        s = RF.scenes()["shape_%dx%d" % (w, h)]
        fr = frames(s.name, sincosf)
        assert fr[0].shape == (1, h, w, 3)
        body = lambda img, e: any(has(img, c) for c in list(s.fill[e]) + list(s.line[e]))
        assert body(fr[0][0], 0), s.name
        if len(fr) > 1:
            assert fr[1].shape == (5, h, w, 3) and body(fr[1][0], 1) and body(fr[1][4], 0), s.name
            assert np.array_equal(fr[1][4], fr[0][0])                                   # the same creature, the same camera
            if w * h > 4:
                assert not np.array_equal(fr[1][0], fr[1][2])                           # the same creature, another camera
        if w >= 64:
            assert len(np.unique(fr[0].reshape(-1, 3), axis=0)) >= 8


@pytest.mark.parametrize("name", list(TF.TERRAINS))
def test_terrain_scenes_show_ground_ends_and_boxes(name, sincosf):
    s = RF.scenes()["terrain_" + name]
    fr = frames(s.name, sincosf)[0]
    cams = s.calls[0][3]
    xs = s.profile.f32()[0]
    for k, img in enumerate(fr):
        assert has(img, M.EDGE_EVEN, 20) and has(img, M.EDGE_ODD, 20), (name, k)
    # (hardcore4 runs below y = 0 for most of its length: lines without ground)
    assert sum(has(img, M.GROUND, 1000) for img in fr) >= (1 if name == "hardcore4" else len(fr))
    # the first view starts left of xs[0], the second ends right of xs[-1]: columns without any ground
    left = int(np.ceil((xs[0] - cams[0][0]) / PX)) - 2
    assert left > 40 and not has(fr[0][:, :left], M.GROUND) and has(fr[0][:, left + 4:], M.GROUND, 1000)
    right = int(np.floor((xs[-1] - cams[1][0]) / PX)) + 2
    assert right < RF.W0 - 40 and not has(fr[1][:, right:], M.GROUND) and (has(fr[1][:, :right - 4], M.GROUND, 1000) or name == "hardcore4")
    assert not has(fr[1][:, right:], M.EDGE_EVEN) and not has(fr[1][:, right:], M.EDGE_ODD)
    if len(s.profile.polys):
        assert has(fr[-1], M.OBST_FILL, 100) and has(fr[-1], M.OBST_LINE, 100)
