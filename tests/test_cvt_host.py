"""Centroid archives and the iso+line emitter without a GPU (include/rem2d_cvt.h): the header's example, the numpy model against an
independent float64 brute force, the forge the GPU file reuses shown to hold what it claims, every wrong variant of the model
visible on it, the line model tied to elites_model's emission, the insertion tied to elites_model's, cvt_centroids on the CPU, the
header, the ctypes binding and the three libraries in agreement, the argument checks of the entry points and the value errors of
the Python layer.

The GPU half (tests/test_cvt_gpu.py) compares the kernels with tests/cvt_model.py bit for bit; this half makes sure that the model
is no vacuous yardstick."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cvt_model as VM
import elites_model as QM
import evolve_model as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
nan, inf = np.nan, np.inf
SMALL = ((14, 1), (1,), (1, 1), (1,))                      # the smallest policy shape: MB 1, R 0, H 1
MID = ((20, 3), (3,), (3, 2), (2,))
WIDTHS, CELLS = (1, 3, 8, 32), (1, 2, 65, 257)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---------------------------------------------------------------------------------------------------- the header's example
def test_the_headers_example():
    cen, rows = np.array([[0], [2], [2], [10]], f32), np.array([[1], [2], [7], [nan]], f32)
    for fn in (VM.assign_model, VM.assign_reference):
        cell, dist = fn(rows, cen)
        assert cell.tolist() == [0, 1, 3, -1] and dist.tolist() == [1.0, 0.0, 9.0, inf]
    with open(os.path.join(ROOT, "include", "rem2d_cvt.h")) as f:
        text = " ".join(re.sub(r"\n \*(?!/)", "\n", f.read()).split())              # (the comment's frame of stars gone)
    assert "centroids = [0, 2, 2, 10], rows = [1, 2, 7, NaN] give cell = [0, 1, 3, -1] and dist = [1, 0, 9, inf]" in text
    for sentence in ("d2 = 0.0f; for i ascending: t = x_i - y_i; d2 = d2 + (t * t)",
                     "best = -1, bestd = +inf; for q = 0 .. C - 1 ascending: if d2(x, c_q) < bestd then best = q, bestd = d2",
                     "child = (x1 + (sigma_iso * z)) + (a * (x2 - x1))", "(0, c, generation, 10)", "(0, c, generation, 11)",
                     "(0, c, generation, 12)", "CPU twin has no counterpart", "12 M C + 8 R",
                     "that table could not be extended when they were added"):
        assert sentence in text, sentence


# --------------------------------------------------------------------------------------------- the model against float64
@pytest.mark.parametrize("B", WIDTHS)
def test_assign_model_against_float64(B):
    """small-integer-valued rows and centroids: every difference, square and sum is exact in binary32 and in binary64, so an
    independent brute force in float64 must give the same cells and the same distances"""
    for C_ in CELLS:
        rng = np.random.default_rng([B, C_, 5])
        rows, cen = rng.integers(-9, 10, (200, B)).astype(f32), rng.integers(-9, 10, (C_, B)).astype(f32)
        d = ((rows.astype(f64)[:, None, :] - cen.astype(f64)[None, :, :]) ** 2).sum(axis=2)
        assert d.max() < 2 ** 24
        want = np.argmin(d, axis=1)
        cell, dist = VM.assign_model(rows, cen)
        assert np.array_equal(cell, want) and np.array_equal(dist.astype(f64), d[np.arange(200), want]), (B, C_)
        assert C_ < 65 or B > 3 or len(set(np.round(d[0]).tolist())) < C_        # (ties are there: the lowest centroid is a choice)


def test_the_package_host_route_is_the_model():
    """elites.assign_host (what cvt_centroids and a CPU archive run) == cvt_model.assign_model == the rule word for word, on bits,
    on the forge, in row chunks of every size"""
    from gym_rem2d_amd import elites
    for B, C_ in ((1, 2), (3, 65), (8, 257), (32, 65)):
        rows, cen = VM.forge(B, C_, 67)
        cell, dist = VM.assign_model(rows, cen)
        ref = VM.assign_reference(rows, cen)
        assert np.array_equal(cell, ref[0]) and np.array_equal(bits(dist), bits(ref[1])), (B, C_)
        for chunk in (None, 1, 5, 67):
            got = elites.assign_host(rows, cen, chunk)
            assert np.array_equal(got[0], cell) and np.array_equal(bits(got[1]), bits(dist)), (B, C_, chunk)


# ------------------------------------------------------------------------------------------------------------- the forge
def test_the_forge_holds_what_it_claims():
    """from the model alone: exact ties between two and among three centroids, duplicate centroids, rows equal to a centroid (one
    with -0 against +0), rows with NaN and +-inf words, a NaN centroid, overflowing differences, denormals, rows without a cell;
    and the all-NaN table, where every cell is -1"""
    total = {}
    for B in WIDTHS:
        for C_ in CELLS:
            for n in (6, 201):
                rows, cen = VM.forge(B, C_, n)
                facts = VM.forge_facts(rows, cen)
                for k, v in facts.items():
                    total[k] = total.get(k, 0) + v
                if n == 201 and C_ >= 65:
                    assert facts["tie2"] + facts["tie3"] >= 1 and facts["duplicates"] >= 1 and facts["equal"] >= 2 and facts["minus_zero"] >= 1, (B, C_, facts)
                    assert facts["nan_rows"] >= 1 and facts["inf_rows"] >= 2 and facts["nan_centroids"] >= 1 and facts["overflow"] >= 1, (B, C_, facts)
                    assert facts["denormal"] >= 2 and facts["no_cell"] >= 3, (B, C_, facts)
                if n == 201 and C_ >= 65 and B >= 2:
                    assert facts["tie2"] >= 1 and facts["tie3"] >= 1, (B, C_, facts)
    assert all(v >= 1 for v in total.values()), total
    rows, cen = VM.forge(8, 65, 201)
    cell, dist = VM.assign_model(rows, np.full_like(cen, nan))
    assert (cell == -1).all() and np.isposinf(dist).all()
    # denormals: the squares underflow to +0, so a denormal row is at distance exactly 0 from the denormal centroid and from (0, ..)
    d2 = VM.d2_model(np.full((1, 2), 1e-40, f32), np.array([[3e-45, 0.0], [0.0, 0.0]], f32))
    assert d2.tolist() == [[0.0, 0.0]] and not np.signbit(d2).any()
    # overflow: the difference is finite and its square is not; 3e38 - (-3e38) is not either
    assert np.isposinf(VM.d2_model(np.array([[3e38], [1e30]], f32), np.array([[-3e38], [0]], f32))).all()


def outputs(rows, cen, variant=None):
    cell, dist = VM.assign_model(rows, cen, variant)
    return np.concatenate([cell.view(np.uint32), bits(dist)])


def line_forge(shapes=MID, C_=9, seed=2):
    """four blocks with 0, 1, 2 and all cells filled; weights with a NaN, a -0 and an inf"""
    rng = np.random.default_rng(seed)
    g = QM.Grid(4, C_, 2, shapes)
    for w in g.weights:
        w[:] = rng.standard_normal(w.shape)
    g.count[1, C_ // 2] = 2
    g.count[2, [1, C_ - 1]] = 1
    g.count[3] = rng.integers(1, 4, C_)
    g.weights[0][3 * C_ + 1, 0, 0], g.weights[2][3 * C_, 0, 0], g.weights[3][-1, 0] = nan, -0.0, inf
    return g


def test_every_mutant_shows_on_the_forge():
    """ties to the highest centroid, `<=` for `<`, a fused multiply-add, an admitted +inf; the line from x2, the second parent drawn
    from the first one's domain, a line coefficient per element: each changes at least one output word.  A mutant the forge cannot
    see is a hole in the forge"""
    rows, cen = VM.forge(8, 65, 201)
    right = outputs(rows, cen)
    shares = {v: float((outputs(rows, cen, v) != right).mean()) for v in VM.ASSIGN_VARIANTS}
    g = line_forge()
    n = 4 * 16
    kids, parent, parent2, n_filled = VM.line_model(g, n, 0.05, 0.3, 11, 4)
    want = np.concatenate([VM.kid_bits(k).ravel() for k in kids] + [parent.view(np.uint32), parent2.view(np.uint32)])
    for v in VM.LINE_VARIANTS:
        k2, p, p2, _ = VM.line_model(g, n, 0.05, 0.3, 11, 4, variant=v)
        got = np.concatenate([VM.kid_bits(k).ravel() for k in k2] + [p.view(np.uint32), p2.view(np.uint32)])
        shares[v] = float((got != want).mean())
    print("share of output words that change: %s" % ", ".join("%s %.2f %%" % (v, 100 * s) for v, s in shares.items()))
    assert set(shares) == set(VM.VARIANTS)
    for v, s in shares.items():
        assert s > 0.0, v


# -------------------------------------------------------------------------------------------------------- the line model
def test_line_model():
    g = line_forge()
    C_, n = g.C, 4 * 16
    before = [np.full((n,) + s, 7.0, f32) for s in MID]
    # sigma_line = +-0 is elites_model.emit_model at threshold 2^32, bit for bit
    for zero in (0.0, -0.0):
        kids, parent, parent2, n_filled = VM.line_model(g, n, 0.05, zero, 11, 4, before=before)
        old, hits, old_parent, old_filled = QM.emit_model(g, n, 2 ** 32, 0.05, 11, 4, before=before)
        assert all(h[16:].all() for h in hits) and np.array_equal(parent, old_parent) and np.array_equal(n_filled, old_filled)
        for k in range(4):
            assert np.array_equal(VM.kid_bits(kids[k]), VM.kid_bits(old[k])), k
    # the first parent is sample_model's; an empty block gives -1 / -1 and untouched children
    kids, parent, parent2, n_filled = VM.line_model(g, n, 0.05, 0.3, 11, 4, before=before)
    assert np.array_equal(parent, QM.sample_model(g.count, n, 11, 4)[1]) and n_filled.tolist() == [0, 1, 2, C_]
    assert (parent[:16] == -1).all() and (parent2[:16] == -1).all() and all((k[:16] == 7.0).all() for k in kids)
    assert (parent[16:32] == C_ + C_ // 2).all() and (parent2[16:32] == C_ + C_ // 2).all()
    assert set(parent2[32:48].tolist()) == {2 * C_ + 1, 3 * C_ - 1} and (parent2[32:] != parent[32:]).any()
    # one filled cell: x2 == x1, the line term is a * 0 and the child is the isotropic one (finite words)
    iso = VM.line_model(g, n, 0.05, 0.0, 11, 4, before=before)[0]
    assert all(np.array_equal(kids[k][16:32], iso[k][16:32]) for k in range(4))
    # one element by hand
    c = 40
    x1, x2 = g.weights[0][parent[c]].ravel()[5], g.weights[0][parent2[c]].ravel()[5]
    w = EM.philox((5, c, 4, 1), EM.seed_key(11))
    z = EM.noise(w[1], w[2], w[3])
    v = EM.philox((0, c, 4, 12), EM.seed_key(11))
    a = f32(0.3) * EM.noise(v[1], v[2], v[3])
    assert kids[0][c].ravel()[5] == f32(f32(x1 + f32(f32(0.05) * z)) + f32(a * f32(x2 - x1)))
    # parent2 is uniform over the filled cells, zl has mean 0 and unit variance: 4096 children over 8 filled cells
    count = np.zeros((1, 20), np.int32)
    filled = [0, 3, 4, 7, 11, 12, 18, 19]
    count[0, filled] = 1
    n_filled, parent, parent2, zl = VM.sample2_model(count, 4096, 77, 9)
    share = np.array([(parent2 == q).mean() for q in filled])
    assert set(parent2.tolist()) == set(filled) and np.abs(share - 1 / 8).max() < 5 / np.sqrt(4096) * np.sqrt(1 / 8 * 7 / 8) + 1e-12, share
    assert np.abs(share - 1 / 8).max() < 5 / np.sqrt(4096)
    assert abs(float(zl.astype(f64).mean())) < 5 / np.sqrt(4096) and abs(float(zl.astype(f64).var()) - 1.0) < 0.15
    assert (parent != parent2).mean() > 0.8                     # (two draws, not one)


# ------------------------------------------------------------------------------------------------------ the insert model
def test_insert_model():
    """on a forged population: elites_model.insert_model fed the model's cells (through a map of C unit cells) gives the same grid,
    cell and winner; a second insertion of the same rows changes nothing"""
    B, C_, M, S = 8, 65, 3, 67
    rows, cen = VM.forge(B, C_, M * S)
    rng = np.random.default_rng(8)
    fitness = rng.integers(-1, 3, M * S).astype(f64)
    fitness[rng.random(M * S) < 0.1] = nan
    fitness[rng.random(M * S) < 0.1] = -0.0
    mask = (rng.random(M * S) < 0.8).astype(np.uint8)
    weights = [rng.standard_normal((M * S,) + s).astype(f32) for s in SMALL]
    grid = QM.Grid(M, C_, B, SMALL)
    grid.count[1], grid.fitness[1] = 1, 1.0
    after, cell, winner, dist = VM.insert_model(cen, grid, weights, fitness, rows, S, mask)
    near, d = VM.assign_model(rows, cen)
    ok = (near >= 0) & ~np.isnan(fitness) & (mask != 0)
    assert np.array_equal(cell, np.where(ok, near, -1)) and np.array_equal(bits(dist), bits(d)) and (~ok).sum() > 10
    fake = np.where(near >= 0, near + 0.5, nan).astype(f32)[:, None]
    want, wcell, wwinner = QM.insert_model(QM.CellMap([0], [C_], [0.0], [1.0]), grid, weights, fitness, fake, S, mask)
    assert np.array_equal(wcell, cell) and np.array_equal(wwinner, winner) and (winner >= 0).sum() > 10 and (winner[1] >= 0).any()
    assert np.array_equal(after.count, want.count) and np.array_equal(bits(after.fitness), bits(want.fitness))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(after.weights, want.weights))
    for b, q in np.argwhere(winner >= 0):
        assert np.array_equal(bits(after.desc[b, q]), bits(rows[winner[b, q]]))
    held = winner < 0
    assert np.array_equal(bits(after.desc[held]), bits(grid.desc[held]))
    again, cell2, winner2, _ = VM.insert_model(cen, after, weights, fitness, rows, S, mask)
    assert np.array_equal(again.words(), after.words()) and (winner2 == -1).all() and np.array_equal(cell2, cell)


# ------------------------------------------------------------------------------------------------------------ centroids
def test_cvt_centroids_on_the_cpu():
    from gym_rem2d_amd import elites
    lo, hi = [0.0, -1.0, 10.0], [1.0, 1.0, 10.5]
    runs = [elites.cvt_centroids(16, lo, hi, n_samples=1024, iterations=k, seed=3).numpy() for k in range(6)]
    again = elites.cvt_centroids(16, lo, hi, n_samples=1024, iterations=5, seed=3).numpy()
    other = elites.cvt_centroids(16, lo, hi, n_samples=1024, iterations=5, seed=4).numpy()
    assert runs[5].dtype == f32 and runs[5].shape == (16, 3)
    assert np.array_equal(bits(again), bits(runs[5])) and not np.array_equal(other, runs[5])
    rng = np.random.Generator(np.random.PCG64(3))
    pts = (np.array(lo, f32) + rng.random((1024, 3), dtype=f32) * (np.array(hi, f32) - np.array(lo, f32))).astype(f32)
    assert np.array_equal(bits(runs[0]), bits(pts[:16]))                        # the start is the first n_cells points
    for c in runs:
        assert (c >= np.array(lo, f32)).all() and (c < np.array(hi, f32)).all()
    err = [float(VM.assign_model(pts, c)[1].astype(f64).mean()) for c in runs]
    print("quantisation error by iteration: %s" % err)
    for a, b in zip(err, err[1:]):
        assert b <= a * (1 + 1e-6), err
    assert err[5] < 0.8 * err[0]
    # one Lloyd step by hand: the mean in binary64 in point order, rounded once
    cell = VM.assign_model(pts, runs[0])[0]
    want = runs[0].copy()
    for q in range(16):
        mine = pts[cell == q].astype(f64)
        if len(mine):
            tot = np.zeros(3)
            for p in mine:
                tot += p
            want[q] = (tot / len(mine)).astype(f32)
    assert np.array_equal(bits(runs[1]), bits(want))
    # an empty cell keeps its centroid: two identical starting points, the second never wins
    same = elites.cvt_centroids(2, [0.0], [1.0], n_samples=2, iterations=3, seed=0)
    assert same.shape == (2, 1)
    for bad in (dict(n_cells=0), dict(n_cells=65537), dict(lo=[0.0, 0.0]), dict(hi=[0.0]), dict(lo=[nan]), dict(n_samples=1), dict(iterations=-1)):
        kw = dict(dict(n_cells=4, lo=[0.0], hi=[1.0], n_samples=16, iterations=1), **bad)
        with pytest.raises(ValueError):
            elites.cvt_centroids(**kw)


# ---------------------------------------------------------------------------------------- header, binding and the libraries
EXPORTS = ["rem2d_cvt_abi_version", "rem2d_cvt_scratch_bytes", "rem2d_cvt_assign", "rem2d_cvt_insert", "rem2d_cvt_emit_line"]


def test_header_binding_and_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    with open(os.path.join(ROOT, "include", "rem2d_cvt.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*(?:int|int64_t)\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert declared == EXPORTS
    assert not re.search(r"\(([^;{}()]*void\s*\*\s*stream[^;{}()]*)\)\s*;", text)          # the stream is a member, not a parameter
    assert int(re.search(r"#define REM2D_CVT_ABI_VERSION (\d+)", text).group(1)) == _lib.CVT_ABI_VERSION == 1
    for name, value in (("MAX_WIDTH", _lib.CVT_MAX_WIDTH), ("MAX_CELLS", _lib.CVT_MAX_CELLS), ("MAX_SPLITS", _lib.CVT_MAX_SPLITS)):
        assert int(re.search(r"#define REM2D_CVT_%s (\d+)" % name, text).group(1)) == value
    body = re.search(r"typedef struct rem2d_cvt \{(.*?)\} rem2d_cvt;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = re.findall(r"^\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+);", body, flags=re.M)
    assert [m[2] for m in members] == [n for n, _ in _lib.Cvt._fields_], members
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
    for (tname, star, name), (_, ct) in zip(members, _lib.Cvt._fields_):
        assert ct is (C.c_void_p if star else ctype[tname]), name
    assert C.sizeof(_lib.Cvt) == 14 * 4 + 8 + 26 * 8 + 8 + 8 and _lib.Cvt.seed.offset == 56 and _lib.Cvt.stream.offset == C.sizeof(_lib.Cvt) - 8
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in declared:
            assert (" T " + name) in syms, (path, name)
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        assert L.rem2d_cvt_abi_version() == _lib.CVT_ABI_VERSION and L.rem2d_abi_version() == 11 and L.rem2d_elites_abi_version() == 1
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):                         # the older headers know nothing of it
        if header == "rem2d_cvt.h":
            continue
        with open(os.path.join(ROOT, "include", header)) as f:
            other = f.read()
        for name in declared + ["REM2D_CVT_", "rem2d_cvt"]:
            assert name not in other, (header, name)


POINTERS = ("centroids", "desc", "fitness", "mask", "w1", "b1", "w2", "b2", "elite_fitness", "elite_desc", "elite_w1", "elite_b1", "elite_w2",
            "elite_b2", "count", "cell", "dist", "winner", "child_w1", "child_b1", "child_w2", "child_b2", "parent", "parent2", "n_filled", "scratch")
AT = {k: (i + 1) << 26 for i, k in enumerate(POINTERS)}      # the "device pointers", 64 MB apart
G_, M_, S_, C_, B_, D_, H_, MB_, R_ = 64, 4, 16, 16, 8, 114, 32, 16, 100
LEN = dict(w1=D_ * H_, b1=H_, w2=H_ * MB_, b2=MB_)
NEED = 12 * M_ * C_ + 8 * R_


def _desc(**kw):
    """a good descriptor: 4 blocks of 16 rows of 8 words, 16 centroids, the workload's policy shape, 64 children, 100 rows to
    assign; the "device pointers" are never dereferenced: the checks come first"""
    from gym_rem2d_amd import _lib
    v = _lib.Cvt()
    v.d, v.hidden, v.max_bodies, v.width, v.n_cells, v.n_blocks, v.group_size, v.n_children, v.n_rows, v.splits = D_, H_, MB_, B_, C_, M_, S_, G_, R_, 0
    v.generation, v.sigma_iso, v.sigma_line, v.reserved, v.seed = 3, 0.01, 0.2, 0, 2 ** 64 - 1
    for k in POINTERS:
        setattr(v, k, AT[k])
    v.scratch_bytes, v.stream = NEED, None
    for k, x in kw.items():
        setattr(v, k, x)
    return v


ASSIGN_SHAPES = [(dict(width=0), b"width"), (dict(width=33), b"width"), (dict(n_cells=0), b"n_cells"), (dict(n_cells=65537), b"n_cells"),
                 (dict(splits=-1), b"splits"), (dict(splits=4097), b"splits"), (dict(reserved=1), b"reserved")]
SHAPES = ASSIGN_SHAPES + [(dict(max_bodies=0), b"max_bodies"), (dict(max_bodies=65), b"max_bodies"), (dict(hidden=0), b"hidden"), (dict(hidden=129), b"hidden"),
                          (dict(d=103), b"d must be"), (dict(d=169), b"d must be"), (dict(n_blocks=0), b"n_blocks"),
                          (dict(n_blocks=32768, n_cells=65536), b"n_blocks times n_cells"), (dict(n_blocks=2 ** 16, group_size=2 ** 15, n_cells=1), b"n_blocks * group_size"),
                          (dict(sigma_iso=nan), b"sigma_iso"), (dict(sigma_line=inf), b"sigma_line")]
SCRATCH = [(dict(scratch=None), b"NULL device pointer (scratch)"), (dict(scratch=AT["scratch"] + 4), b"8-byte aligned"), (dict(scratch_bytes=0), b"scratch holds")]
ROWS = ([(dict(**{k: None}), ("NULL device pointer (%s)" % k).encode()) for k in ("centroids", "desc", "cell")]
        + [(dict(desc=AT["cell"]), b"desc overlaps cell"), (dict(centroids=AT["dist"]), b"centroids overlaps dist"), (dict(desc=AT["dist"] + 4), b"desc overlaps dist")])
ASSIGN = ASSIGN_SHAPES + SCRATCH + ROWS + [(dict(n_rows=0), b"n_rows"), (dict(n_rows=-5), b"n_rows"), (dict(scratch_bytes=8 * R_ - 1), b"scratch holds")]
INSERT = (SHAPES + SCRATCH + ROWS + [(dict(group_size=0), b"group_size"), (dict(group_size=-16), b"group_size"), (dict(scratch_bytes=12 * M_ * C_ + 8 * G_ - 1), b"scratch holds")]
          + [(dict(**{k: None}), ("NULL device pointer (%s)" % k).encode()) for k in ("fitness", "elite_fitness", "elite_desc", "count", "winner")]
          + [(dict(**{k: None}), b"NULL device pointer (weights)") for k in ("w1", "b1", "w2", "b2", "elite_w1", "elite_b1", "elite_w2", "elite_b2")]
          + [(dict(desc=AT[k]), ("desc overlaps %s" % k).encode()) for k in ("elite_fitness", "elite_desc", "count", "elite_w1", "elite_b1", "elite_w2", "elite_b2")]
          + [(dict(centroids=AT[k]), ("centroids overlaps %s" % k).encode()) for k in ("elite_desc", "count", "elite_w2")]
          + [(dict(w1=AT["elite_w1"]), b"elite_w1 overlaps the evaluated sets' w1"), (dict(b2=AT["elite_w2"] + 64), b"elite_w2 overlaps the evaluated sets' b2")])
LINE = (SHAPES + SCRATCH + [(dict(n_children=0), b"n_children"), (dict(n_children=66), b"n_children"), (dict(scratch_bytes=12 * M_ * C_ - 1), b"scratch holds")]
        + [(dict(**{k: None}), ("NULL device pointer (%s)" % k).encode()) for k in ("count", "parent", "parent2", "n_filled")]
        + [(dict(**{k: None}), b"NULL device pointer (weights)") for k in ("child_w1", "child_b1", "child_w2", "child_b2", "elite_w1", "elite_b1", "elite_w2", "elite_b2")]
        + [(dict(child_w1=AT["elite_w1"]), b"child_w1 overlaps elite_w1"), (dict(child_b2=AT["elite_w2"] + M_ * C_ * LEN["w2"] * 4 - 4), b"child_b2 overlaps elite_w2"),
           (dict(child_w2=AT["elite_b1"] - G_ * LEN["w2"] * 4 + 4), b"child_w2 overlaps elite_b1")])


def test_bad_arguments_are_refused_before_anything_is_dereferenced():
    """Every REM2D_E_INVALID of include/rem2d_cvt.h, in the three builds, on a machine without a GPU: nothing is launched"""
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        err = L.rem2d_last_error
        for fn, prefix, cases in ((L.rem2d_cvt_assign, b"cvt_assign: ", ASSIGN), (L.rem2d_cvt_insert, b"cvt_insert: ", INSERT),
                                  (L.rem2d_cvt_emit_line, b"cvt_emit_line: ", LINE)):
            assert fn(None) == -1 and b"NULL descriptor" in err() and err().startswith(prefix)
            for kw, msg in cases:
                assert fn(C.byref(_desc(**kw))) == -1 and msg in err() and err().startswith(prefix), (prefix, kw, err())
        assert L.rem2d_cvt_scratch_bytes(None) == -1 and err().startswith(b"cvt_scratch_bytes: ")
        for kw, msg in SHAPES:
            assert L.rem2d_cvt_scratch_bytes(C.byref(_desc(**kw))) == -1 and msg in err(), (kw, err())
        assert L.rem2d_cvt_scratch_bytes(C.byref(_desc())) == NEED
        assert L.rem2d_cvt_scratch_bytes(C.byref(_desc(**{k: None for k in POINTERS}))) == NEED            # no pointer is looked at
        assert L.rem2d_cvt_scratch_bytes(C.byref(_desc(n_rows=0, group_size=0))) == 12 * M_ * C_
        assert L.rem2d_cvt_scratch_bytes(C.byref(_desc(n_rows=10))) == 12 * M_ * C_ + 8 * G_
        # assign looks at nothing of the policy shapes or the blocks
        short = dict(scratch_bytes=8 * R_ - 1)
        assert L.rem2d_cvt_assign(C.byref(_desc(d=0, hidden=0, max_bodies=0, n_blocks=0, group_size=0, n_children=0, sigma_iso=nan, **short))) == -1 and b"scratch holds" in err()


# --------------------------------------------------------------------------------------------------------- Python errors
def test_python_layer_errors():
    import torch
    from gym_rem2d_amd import elites, policy
    like = policy.MLPPolicy.random(8, 16, 32)
    cen = np.random.default_rng(0).standard_normal((5, 8)).astype(f32)
    arch = elites.CentroidArchive(2, cen, like=like)
    assert arch.n_cells == 5 and arch.width == 8 and arch.centroids.dtype == torch.float32 and arch.device.type == "cpu"
    assert np.array_equal(arch.centroids.numpy(), cen) and arch.count.shape == (2, 5) and arch.w1.shape[0] == 10
    assert isinstance(arch, elites.EliteGrid) and arch.coverage().tolist() == [0.0, 0.0]
    for bad in (cen.astype(f64), cen[0], np.zeros((0, 8), f32), np.zeros((65537, 1), f32), np.zeros((4, 33), f32), "centroids",
                torch.zeros((4, 8), dtype=torch.float64)):
        with pytest.raises(ValueError):
            elites.CentroidArchive(2, bad, like=like)
    with pytest.raises(ValueError):
        elites.CentroidArchive(0, cen, like=like)
    with pytest.raises(ValueError):
        elites.CentroidArchive(2, cen, like=None)
    # assign on a CPU archive is the host route; its argument checks
    rows = torch.from_numpy(np.random.default_rng(1).standard_normal((7, 8)).astype(f32))
    dist = torch.empty(7)
    cell = arch.assign(rows, dist=dist)
    want = VM.assign_model(rows.numpy(), cen)
    assert np.array_equal(cell.numpy(), want[0]) and np.array_equal(bits(dist.numpy()), bits(want[1]))
    for bad in (rows.double(), rows[:, :7], rows.t(), rows.numpy(), rows[:0]):
        with pytest.raises(ValueError):
            arch.assign(bad)
    for kw in (dict(out=torch.empty(7)), dict(out=torch.empty(6, dtype=torch.int32)), dict(dist=torch.empty(7, dtype=torch.float64)), dict(splits=-1), dict(splits=4097)):
        with pytest.raises(ValueError):
            arch.assign(rows, **kw)
    # insert: EliteGrid's checks, then the refusal of a CPU device
    pop = policy.MLPPolicy.random(8, 16, 32, seed=1)
    fit, desc = torch.zeros(8, dtype=torch.float64), torch.zeros((8, 8))
    indexed = policy.MLPPolicy(pop.w1, pop.b1, pop.w2, pop.b2, index=torch.arange(8))
    for args in ((pop, fit.float(), desc), (pop, fit[:7], desc), (pop, fit, desc.double()), (pop, fit, desc[:, :7]), (indexed, fit, desc),
                 (policy.MLPPolicy.random(8, 16, 16), fit, desc), (like, fit, arch.desc.view(-1, 8)[:8])):
        with pytest.raises(ValueError):
            arch.insert(*args)
    with pytest.raises(ValueError):
        arch.insert(pop, fit, desc, mask=torch.ones(8))
    with pytest.raises(ValueError):
        arch.insert(pop, fit, desc, group_size=3)
    with pytest.raises(ValueError, match="on the GPU"):
        arch.insert(pop, fit, desc)
    # emit_line, on grids and archives alike
    grid = elites.EliteGrid(2, [(0, 0.0, 1.0, 4)], 8, like=like)
    for g in (arch, grid):
        for kw in (dict(generation=-1), dict(generation=2 ** 32), dict(seed=2 ** 64), dict(n_children=3), dict(n_children=0), dict(sigma_iso=nan),
                   dict(sigma_line=inf), dict(out=indexed), dict(out=policy.MLPPolicy.random(8, 16, 16)), dict(out=pop, n_children=6)):
            with pytest.raises(ValueError):
                g.emit_line(**dict(dict(generation=1), **kw))
        with pytest.raises(ValueError, match="on the GPU"):
            g.emit_line(1, n_children=8)
    # a checkpoint carries the centroids
    state = arch.state_dict()
    assert set(state) == {"fitness", "desc", "count", "w1", "b1", "w2", "b2", "centroids"}
    other = elites.CentroidArchive(2, np.zeros((5, 8), f32), like=like)
    other.load_state_dict(state)
    assert np.array_equal(other.centroids.numpy(), cen)
    with pytest.raises(ValueError):
        elites.CentroidArchive(2, np.zeros((6, 8), f32), like=like).load_state_dict(state)
