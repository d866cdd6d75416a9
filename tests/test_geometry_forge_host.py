"""The cases of tests/geometry_forge.py reach what they are for -- on the oracle alone, no GPU.

tests/test_geometry_gpu.py compares the device with the oracle word for word on these tables; that comparison is only as good
as the tables.  Here, from the oracle's answers: every manifold type each narrowphase routine can return appears, point counts
0 / 1 / 2 appear, both outcomes of b2CollidePolygons' flip rule occur, the boundary ladders do straddle their boundary (and the
same ladders moved off it do not), b2TimeOfImpact ends separated / touching / overlapped in numbers, GJK ends with 1, 2 and 3
simplex vertices, and every near-miss sub-family of the exact TOI skip holds >= 25 % pairs that must not be skipped.  Also the
bad-argument table of rem2d_selftest_geometry and the header's names, which need the library but no device.
`pytest -s` prints the coverage table DESIGN.md quotes.
"""
import collections
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import geometry_forge as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def answers(name):
    from oracle import oracle as O
    O.build()
    spec, fam = {"collide": G.collide_cases, "collide_bulk": G.collide_bulk, "distance": G.distance_cases, "toi": G.toi_cases,
                 "near": G.near_miss_cases}[name]()
    op = {"collide_bulk": "collide", "near": "toi"}.get(name, name)
    fo, io, extra = O.geometry_batch(op, spec)
    assert spec.dtype == np.float32 and np.isfinite(spec).all()
    assert np.isfinite(fo).all(), "a case whose oracle output is not finite is a forge error"
    return spec, fam, fo, io, extra


def _both(values):
    return len(set(values.tolist())) > 1


def _changing(fam, values, keep):
    """{family: does `values` take more than one value inside it} over the rows of `keep`, with one pass over the names."""
    names, inv = np.unique(fam[keep], return_inverse=True)
    v = values[keep].astype(np.int64)
    lo, hi = np.full(len(names), np.iinfo(np.int64).max), np.full(len(names), np.iinfo(np.int64).min)
    np.minimum.at(lo, inv, v)
    np.maximum.at(hi, inv, v)
    return dict(zip(names.tolist(), (lo != hi).tolist()))


def test_collide_reaches_every_type_count_and_boundary():
    spec, fam, fo, io, _ = answers("collide")
    pair = np.array([f[:2] for f in fam])
    # manifold types each routine can return: b2CollideEdgeAndCircle circles / faceA, b2EPCollider faceA / faceB,
    # b2CollidePolygons faceA / faceB (= both outcomes of the flip rule), b2CollidePolygonAndCircle faceA
    want_types = {"ec": {0, 1}, "eb": {1, 2}, "bb": {1, 2}, "bc": {1}}
    want_counts = {"ec": {0, 1}, "eb": {0, 1, 2}, "bb": {0, 1, 2}, "bc": {0, 1}}
    is_ladder = (np.char.find(fam, "#") >= 0) | (np.char.find(fam, "~") >= 0)
    count_changes = _changing(fam, io[:, 1], is_ladder)                   # the point count, per ladder and control
    type_changes = _changing(fam, io[:, 0], is_ladder & (io[:, 1] > 0))   # the reference face, where there are points
    for off in G.OFFSETS:
        at = np.char.endswith(fam, "@%g" % off)
        tag = "@%g" % off
        for p in ("eb", "ec", "bb", "bc"):
            m = (pair == p) & at
            hit = m & (io[:, 1] > 0)
            types, counts = collections.Counter(io[hit, 0].tolist()), collections.Counter(io[m, 1].tolist())
            print("collide %s @%g: %6d cases, types %s, counts %s" % (p, off, m.sum(), dict(types), dict(counts)))
            assert set(types) == want_types[p] and min(types.values()) >= 100, (p, off, types)
            assert set(counts) == want_counts[p] and min(counts.values()) >= 100, (p, off, counts)
            # the contact radius exactly: the point count changes inside EVERY ladder, so some pair of neighbouring steps (at
            # most one ulp apart in either coordinate) has both outcomes; inside no control off the boundary
            ids = sorted(f for f in count_changes if f.startswith(p + "/radius#") and f.endswith(tag))
            straddle = [f for f in ids if count_changes[f]]
            ctl = [f for f in count_changes if f.startswith(p + "/radius~") and f.endswith(tag) and count_changes[f]]
            print("   radius ladders %d, count changes inside %d, inside a control %d" % (len(ids), len(straddle), len(ctl)))
            assert len(ids) >= 20 and len(straddle) == len(ids) and not ctl, (p, off, sorted(set(ids) - set(straddle))[:5])
            if p in ("eb", "bb"):   # the clips keep two, one and zero points
                assert set(io[m & np.char.startswith(fam, p + "/clip"), 1].tolist()) == {0, 1, 2}
        # the flip rule's boundary: the reference face changes sides inside every ladder, never inside its control 2 cm away
        ids = sorted(f for f in type_changes if f.startswith("bb/flip#") and f.endswith(tag))
        flips = [f for f in ids if type_changes[f]]
        ctl = [f for f in type_changes if f.startswith("bb/flip~") and f.endswith(tag) and type_changes[f]]
        print("flip ladders @%g: %d, type changes inside %d, inside a control %d" % (off, len(ids), len(flips), len(ctl)))
        assert len(ids) >= 30 and len(flips) == len(ids) and not ctl
    # region families: A, B and AB of the edge-circle routine by feature key (vertex 0, vertex 1, face)
    ec = (pair == "ec") & (io[:, 1] > 0)
    keys = set((io[ec, 2] & 0xffffff).tolist())
    assert keys == {0x000000, 0x000001, 0x010000}, keys
    spec2, fam2, fo2, io2, _ = answers("collide_bulk")
    assert set(io2[:, 1].tolist()) == {0, 1, 2} and 0.2 < (io2[:, 1] > 0).mean() < 0.9


def test_boundaries_are_met_to_the_bit():
    """The branch boundaries the cases are placed on are HIT, shown by restating the deciding quantity in binary32 (numpy
    float32 operations round one by one, like the routines) or by reading it from the oracle."""
    from oracle import oracle as O
    f = np.float32
    spec, fam, fo, io, _ = answers("collide")
    pair = np.array([x[:2] for x in fam])
    # b2CollideEdgeAndCircle: u = e . (B - Q), v = e . (Q - A) exactly 0 (the centre on the perpendicular through an end point)
    m = pair == "ec"
    A, B, Q = spec[m, 1:3], spec[m, 3:5], spec[m, 12:14]
    e = B - A
    u = e[:, 0] * (B - Q)[:, 0] + e[:, 1] * (B - Q)[:, 1]
    v = e[:, 0] * (Q - A)[:, 0] + e[:, 1] * (Q - A)[:, 1]
    hit = io[m, 1] > 0
    print("edge-circle: u == 0 in %d cases (%d touching), v == 0 in %d (%d)" % ((u == 0).sum(), ((u == 0) & hit).sum(), (v == 0).sum(), ((v == 0) & hit).sum()))
    assert ((u == 0) & hit).sum() >= 10 and ((v == 0) & hit).sum() >= 10
    assert ((u == 0) & hit & (io[m, 0] == 0)).any() and ((v == 0) & hit & (io[m, 0] == 0)).any()      # u <= 0 / v <= 0: vertex regions
    # ... dd == rr: the triple (-1 ulp, exact, +1 ulp) around it gives one point, one point, none
    t = np.char.startswith(fam, "ec/dd_eq_rr")
    end = np.where(spec[t, 12] == spec[t, 1], 0, 2)
    d = spec[t, 12:14] - np.stack((spec[t, 1 + end], spec[t, 2 + end]), 1)
    dd, rr = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1], (f(0.01) + spec[t, 10]) * (f(0.01) + spec[t, 10])
    assert t.sum() == 72 and (dd == rr).sum() == 24 and (dd < rr).sum() == 24 and (dd > rr).sum() == 24
    assert (io[t, 1] == np.where(dd > rr, 0, 1)).all() and (io[t, 0][dd <= rr] == 0).all()
    # b2CollidePolygonAndCircle: u1 / u2 exactly 0 on a touched face (the centre level with a corner of the hardcore box)
    m = (pair == "bc") & (io[:, 1] > 0)
    xs, ys = spec[m, 1:9:2], spec[m, 2:9:2]
    c = spec[m, 12:14]
    V = np.stack((np.stack((xs.max(1), ys.min(1)), 1), np.stack((xs.max(1), ys.max(1)), 1), np.stack((xs.min(1), ys.max(1)), 1),
                  np.stack((xs.min(1), ys.min(1)), 1)), 1)             # the hull order rem2d_selftest_static_box returns
    zero1 = zero2 = 0
    for i in range(4):
        v1, v2 = V[:, i], V[:, (i + 1) % 4]
        on = (fo[m, 2] == f(0.5) * (v1 + v2)[:, 0]) & (fo[m, 3] == f(0.5) * (v1 + v2)[:, 1]) | ((fo[m, 2:4] == v1).all(1)) | ((fo[m, 2:4] == v2).all(1))
        u1 = ((c - v1) * (v2 - v1)).astype(f)
        u2 = ((c - v2) * (v1 - v2)).astype(f)
        zero1 += int(((u1[:, 0] + u1[:, 1] == 0) & on).sum())
        zero2 += int(((u2[:, 0] + u2[:, 1] == 0) & on).sum())
    print("box-circle: u1 == 0 in %d touching cases, u2 == 0 in %d" % (zero1, zero2))
    assert zero1 >= 10 and zero2 >= 10
    # b2CollidePolygons: separationA == separationB (aligned boxes), and the flip rule's tie to the bit
    m = (pair == "bb") & (io[:, 1] > 0)
    sep = O.polygon_separations(spec[m])
    print("box-box: separationA == separationB in %d touching cases" % (sep[:, 0] == sep[:, 1]).sum())
    assert (sep[:, 0] == sep[:, 1]).sum() >= 100
    ties = G.flip_ties()
    sep = O.polygon_separations(ties)
    tf, ti, _ = O.geometry_batch("collide", ties)
    assert len(ties) >= 10 and (sep[:, 1] == sep[:, 0] + f(0.1) * f(0.005)).all() and (sep[:, 1] != sep[:, 0]).all()
    assert (ti[:, 1] > 0).all() and (ti[:, 0] == 1).all()          # `>`: a tie keeps the hardcore box's face (e_faceA)
    # and one ulp more of separationB would flip: both outcomes stand either side of each tie in its ladder family above


def test_distance_reaches_every_simplex():
    spec, fam, fo, io, iters = answers("distance")
    counts = collections.Counter(io[:, 0].tolist())
    print("distance: %d cases, simplex counts %s, iterations %s" % (len(spec), dict(counts), dict(collections.Counter(iters.tolist()))))
    assert set(counts) == {1, 2, 3} and min(counts.values()) >= 1000
    base = np.array([f.split("@")[0] for f in fam])
    for name in ("vertex_on_line", "overlap", "parallel", "collinear", "beyond", "bulk"):
        assert (base == name).sum() >= 100, name
    boxes = spec[:, 9] == 1          # (a circle's core is a point: under an edge's line it does not overlap the edge; a turned
    assert (fo[(base == "overlap") & boxes, 0] == 0).mean() > 0.8      # box's low corner can hang beyond a short edge's end)
    assert (fo[base == "vertex_on_line", 0] == 0).any() and (fo[base == "vertex_on_line", 0] > 0).any()
    assert (fo[base == "beyond", 0] > 0).mean() > 0.5         # (a wide box half a face beyond an end still reaches over it)
    assert iters.max() >= 3       # the largest the search finds is printed above and recorded in DESIGN.md


def test_toi_reaches_every_state():
    spec, fam, fo, io, _ = answers("toi")
    states = collections.Counter(G.TOI_STATES[s] for s in io[:, 0].tolist())
    print("toi: %d cases, states %s (failed found: %s)" % (len(spec), dict(states), "failed" in states))
    for s in ("separated", "touching", "overlapped"):
        assert states[s] >= 500, states
    assert "unknown" not in states
    base = np.array([f.split("@")[0] for f in fam])
    touch = io[:, 0] == 3
    assert touch[base == "drop"].all() and touch[base == "through"].all()         # tunnelling is stopped
    boxes = spec[:, 9] == 1          # (a circle's core is a point: it overlaps a hardcore box, never an edge)
    assert (io[(base == "overlapped0") & boxes, 0] == 2).mean() > 0.9 and (io[base == "overlapped0", 0] == 2).sum() >= 500
    assert (touch & (fo[:, 0] == 0))[base == "touching0"].any()
    assert _both(io[base == "slide", 0]) and _both(io[base == "rotate", 0]) and _both(io[base == "end", 0])
    for s in ("turns", "shared_vertex", "many_turns"):
        assert touch[base == s].sum() >= 20, s


def test_near_miss_families_hold_pairs_that_must_not_be_skipped():
    spec, fam, fo, io, _ = answers("near")
    event = (io[:, 0] == 3) & (fo[:, 0] < 1.0)
    names = sorted(set(fam.tolist()))
    assert len(names) == len(G.NEAR_PASSES) * len(G.NEAR_MOTIONS) * 2 * len(G.OFFSETS)
    for f in names:
        m = fam == f
        print("%-34s %3d cases, %2d events, states %s" % (f, m.sum(), event[m].sum(), dict(collections.Counter(io[m, 0].tolist()))))
        assert m.sum() == 48 and event[m].mean() >= 0.25, f
        assert (~event[m]).sum() >= 12, f      # ... and pairs the skip may take


def test_library_exports_the_selftest_header():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    with open(os.path.join(ROOT, "include", "rem2d_selftest.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*int\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert set(declared) == {"rem2d_selftest_abi_version", "rem2d_selftest_static_box", "rem2d_selftest_geometry"}
    for name, value in (("REM2D_SELFTEST_ABI_VERSION", _lib.SELFTEST_ABI_VERSION), ("REM2D_SELFTEST_CASE_WORDS", _lib.SELFTEST_CASE_WORDS),
                        ("REM2D_SELFTEST_OUT_WORDS", _lib.SELFTEST_OUT_WORDS)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    assert (_lib.SELFTEST_CASE_WORDS, _lib.SELFTEST_OUT_WORDS) == (G.DEVICE_WORDS, G.OUT_WORDS)
    ops = re.findall(r"REM2D_SELFTEST_([A-Z_]+) = (\d)", text)
    assert [(n.lower(), int(v)) for n, v in ops[:4]] == list(zip(_lib.SELFTEST_OPS, range(4)))
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in declared:
            assert (" T " + name) in syms, (path, name)
    for wide in (False, True, "fma"):
        assert _lib.lib(wide).rem2d_selftest_abi_version() == _lib.SELFTEST_ABI_VERSION
    with open(os.path.join(ROOT, "include", "rem2d.h")) as f:      # the pinned header knows nothing of it
        assert "rem2d_selftest_geometry" not in f.read()


def test_bad_arguments_are_refused_before_anything_is_dereferenced():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    L = _lib.lib()
    err, S = L.rem2d_last_error, L.rem2d_selftest_geometry
    buf = C.c_void_p(256)      # a "device pointer" that is never dereferenced: the argument checks come first
    table = (
        ((-1, 1, buf, 26, buf, buf, 0, None), b"unknown op"),
        ((4, 1, buf, 26, buf, buf, 0, None), b"unknown op"),
        ((0, -1, buf, 26, buf, buf, 0, None), b"n < 0"),
        ((0, 1, buf, 25, buf, buf, 0, None), b"case_words"),
        ((0, 1, buf, 0, buf, buf, 0, None), b"case_words"),
        ((2, 1, None, 26, buf, buf, 0, None), b"NULL device pointer"),
        ((2, 1, buf, 26, None, buf, 0, None), b"NULL device pointer"),
        ((3, 1, buf, 26, buf, None, 0, None), b"NULL device pointer"),
    )
    for args, msg in table:
        assert S(*args) == -1 and msg in err(), (args, err())
    assert S(1, 0, None, 26, None, None, 0, None) == 0          # n = 0 is a no-op, whatever the pointers
    # the host-only box derivation: the terrain upload's own code (vertex order and normals are part of what is tested)
    out = np.zeros(16, np.float32)
    assert L.rem2d_selftest_static_box(None, out.ctypes.data) == -1 and L.rem2d_selftest_static_box(out.ctypes.data, None) == -1
    assert L.rem2d_selftest_static_box(out.ctypes.data, out.ctypes.data) == -1 and b"convex quad" in err()    # four equal corners
    xy = np.array([10, 5, 11, 5, 11, 6, 10, 6], np.float32)
    assert L.rem2d_selftest_static_box(xy.ctypes.data, out.ctypes.data) == 0
    assert out[:8].tolist() == [11, 5, 11, 6, 10, 6, 10, 5] and out[8:].tolist() == [1, 0, 0, 1, -1, 0, 0, -1]


def test_static_box_matches_the_oracles_polygon():
    """The vertices the library derives for every hardcore box of the forge are the ones the oracle's b2PolygonShape::Set holds:
    checked through the manifold's local point of a circle resting on each face (b2CollidePolygonAndCircle returns the face's
    end points' mean)."""
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    box = G.library_static_box(_lib.lib())
    spec, fam, fo, io, _ = answers("collide")
    m = (spec[:, 0] == 1) & (spec[:, 9] == 2) & (io[:, 1] == 1)
    seen = 0
    for raw in np.unique(spec[m, 1:9], axis=0):
        v = box(np.ascontiguousarray(raw))[:8].reshape(4, 2)
        mids = {tuple((np.float32(0.5) * (v[i] + v[(i + 1) % 4])).tolist()) for i in range(4)} | {tuple(p) for p in v.tolist()}
        rows = m & (spec[:, 1:9] == raw).all(axis=1)
        assert {tuple(p) for p in fo[rows, 2:4].tolist()} <= mids
        seen += 1
    assert seen >= 6
