"""Centroid archives and the iso+line emitter stated on the host (include/rem2d_cvt.h), shared by tests/test_cvt_host.py (numpy alone)
and tests/test_cvt_gpu.py: what elites_model.py is for the regular grids.  Written from the header, not from the kernels.

* ``assign_model``: (cell int32 [n], dist float32 [n]) -- the nearest centroid of every row, binary32 operation by operation.
* ``insert_model``: the insertion; everything after the cell is elites_model.insert_model itself.
* ``sample2_model``: (n_filled, parent, parent2, a) -- the two draws and the line coefficient of every child.
* ``line_model``: the children.
* ``forge``: the rows and centroids both test files use: ties, duplicates, +-0, NaN, +-inf, overflow, denormals.

The ``variant`` names state WRONG rules, for the mutant test of test_cvt_host.py.
"""
import numpy as np

import elites_model as QM
import evolve_model as EM
from evolve_model import philox, seed_key

f32, f64 = np.float32, np.float64
u32, u64 = np.uint32, np.uint64
inf, nan = f32(np.inf), f32(np.nan)
DOMAIN1, DOMAIN2, DOMAIN_A = QM.ELITES_DOMAIN, 11, 12       # the first parent (the grid header's draw), the second, the coefficient
ASSIGN_VARIANTS = ("ties_highest", "le", "fused", "admit_inf")
LINE_VARIANTS = ("line_from_x2", "same_domain", "a_per_element")
VARIANTS = ASSIGN_VARIANTS + LINE_VARIANTS


# ------------------------------------------------------------------------------------------------------------------ assign
def d2_model(desc, centroids, variant=None):
    """float32 [n, C]: d2 = d2 + (t * t), t = x_i - y_i, i ascending, every operation rounded to binary32"""
    x, y = np.ascontiguousarray(desc, f32), np.ascontiguousarray(centroids, f32)
    assert x.ndim == 2 and y.ndim == 2 and x.shape[1] == y.shape[1]
    d2 = np.zeros((x.shape[0], y.shape[0]), f32)
    with np.errstate(all="ignore"):
        for i in range(x.shape[1]):
            t = x[:, i, None] - y[None, :, i]
            assert t.dtype == f32
            if variant == "fused":                             # fma(t, t, d2): the product exact in binary64, one rounding to binary32
                d2 = (t.astype(f64) * t.astype(f64) + d2.astype(f64)).astype(f32)
            else:
                p = t * t
                assert p.dtype == f32
                d2 = d2 + p
            assert d2.dtype == f32
    return d2


def assign_model(desc, centroids, variant=None):
    """best = -1, bestd = +inf; for q ascending: if d2 < bestd then best = q, bestd = d2 -> (cell int32 [n], dist float32 [n])"""
    assert variant is None or variant in VARIANTS
    d2 = d2_model(desc, centroids, variant)
    n, C = d2.shape
    rows = np.arange(n)
    if variant == "le":                                        # `<=`: the LAST of the equal minima, and +inf passes
        d = np.where(np.isnan(d2), inf, d2)
        q = C - 1 - np.argmin(d[:, ::-1], axis=1)
        some = ~np.isnan(d2).all(axis=1)
        best = d[rows, q]
        # (an all-inf row: q is the last centroid that is not a NaN)
        lastok = C - 1 - np.argmax(~np.isnan(d2)[:, ::-1], axis=1)
        q = np.where(best == inf, lastok, q)
        return np.where(some, q, -1).astype(np.int32), np.where(some, best, inf).astype(f32)
    if variant == "admit_inf":                                 # a +inf candidate is chosen where nothing finite is there
        d = np.where(np.isnan(d2), inf, d2)
        q = np.argmin(d, axis=1)
        best = d[rows, q]
        firstok = np.argmax(~np.isnan(d2), axis=1)
        q = np.where(best == inf, firstok, q)
        some = ~np.isnan(d2).all(axis=1)
        return np.where(some, q, -1).astype(np.int32), np.where(some, best, inf).astype(f32)
    d = np.where(np.isfinite(d2), d2, inf)
    if variant == "ties_highest":
        q = C - 1 - np.argmin(d[:, ::-1], axis=1)
    else:
        q = np.argmin(d, axis=1)                               # the first of the equal minima
    best = d[rows, q]
    return np.where(best < inf, q, -1).astype(np.int32), best.astype(f32)


def assign_reference(desc, centroids):
    """the sequential rule word for word, one row and one centroid at a time (slow; for small inputs)"""
    x, y = np.ascontiguousarray(desc, f32), np.ascontiguousarray(centroids, f32)
    cell, dist = np.full(len(x), -1, np.int32), np.full(len(x), inf, f32)
    with np.errstate(all="ignore"):
        for r in range(len(x)):
            best, bestd = -1, inf
            for q in range(len(y)):
                d2 = f32(0.0)
                for i in range(x.shape[1]):
                    t = f32(x[r, i] - y[q, i])
                    d2 = f32(d2 + f32(t * t))
                if d2 < bestd:
                    best, bestd = q, d2
            cell[r], dist[r] = best, bestd
    return cell, dist


# ------------------------------------------------------------------------------------------------------------------ insert
def insert_model(centroids, grid, weights, fitness, desc, group_size, mask=None, variant=None):
    """-> (grid after, cell int32 [G], winner int32 [M, C], dist float32 [G]); the inputs are not written.  The cell is the nearest
    centroid; the admission by fitness and mask, the challenger, the strict replacement, count, winner and the copies are
    elites_model.insert_model's, which is handed a one-word row per population row that lands in that cell (q + 1/2 on a map of C
    unit cells; a NaN where there is none)"""
    desc = np.ascontiguousarray(desc, f32)
    C = grid.C
    assert C == len(centroids) <= QM.MAX_CELLS
    near, dist = assign_model(desc, centroids, variant)
    stand_in = np.where(near >= 0, near.astype(f32) + f32(0.5), nan).astype(f32)[:, None]
    assert np.array_equal(np.where(near >= 0, np.trunc(stand_in[:, 0]), -1), near)          # exact below 2^16
    cmap = QM.CellMap([0], [C], [0.0], [1.0])
    out, cell, winner = QM.insert_model(cmap, grid, weights, fitness, stand_in, group_size, mask)
    took = np.argwhere(winner >= 0)
    for b, q in took:                                          # (the descriptor row that is kept is the real one)
        out.desc[b, q] = desc[winner[b, q]]
    return out, cell, winner, dist


# -------------------------------------------------------------------------------------------------------------- the draws
def sample2_model(count, n_children, seed, generation, variant=None):
    """count int32 [M, C] -> (n_filled int32 [M], parent int32 [n], parent2 int32 [n], zl float32 [n]): the grid header's draw
    (domain 10), the second parent's (domain 11) and the unit draw of the line coefficient (domain 12, x1 .. x3)"""
    count = np.asarray(count)
    M, C = count.shape
    n_filled, parent = QM.sample_model(count, n_children, seed, generation)
    per = int(n_children) // M
    c = np.arange(n_children, dtype=np.int64)
    key = seed_key(seed)
    x0 = philox((0, c, generation, DOMAIN1 if variant == "same_domain" else DOMAIN2), key)[0].astype(u64)
    parent2 = np.full(n_children, -1, np.int32)
    for b in range(M):
        f = np.flatnonzero(count[b] != 0)
        if len(f) == 0:
            continue
        j = ((x0[b * per:(b + 1) * per] * u64(len(f))) >> u64(32)).astype(np.int64)
        parent2[b * per:(b + 1) * per] = b * C + f[j]
    _, x1, x2, x3 = philox((0, c, generation, DOMAIN_A), key)
    return n_filled, parent, parent2, EM.noise(x1, x2, x3)


def line_model(grid, n_children, sigma_iso, sigma_line, seed, generation, before=None, variant=None):
    """-> (children: four arrays [n_children, ...], parent, parent2, n_filled).  child = (x1 + (sigma_iso * z)) + (a * (x2 - x1)),
    a = sigma_line * zl; sigma_line == +-0: child = x1 + (sigma_iso * z).  A child whose parents are -1 keeps what ``before``
    (four arrays, default zeros) holds"""
    assert variant is None or variant in VARIANTS
    n_filled, parent, parent2, zl = sample2_model(grid.count, n_children, seed, generation, variant)
    kids = [np.zeros((n_children,) + a.shape[1:], f32) if before is None else np.array(before[k], f32) for k, a in enumerate(grid.weights)]
    born = np.flatnonzero(parent >= 0)
    assert np.array_equal(born, np.flatnonzero(parent2 >= 0))
    s_iso, s_line = f32(sigma_iso), f32(sigma_line)
    key = seed_key(seed)
    with np.errstate(all="ignore"):
        a = (s_line * zl[born])[:, None]                      # one binary32 product per child
        assert a.dtype == f32
        for k, arr in enumerate(grid.weights):
            n = int(np.prod(arr.shape[1:], dtype=np.int64))
            flat = arr.reshape(arr.shape[0], n)
            x1, x2 = flat[parent[born]], flat[parent2[born]]
            i = np.arange(n, dtype=np.int64)[None, :]
            _, w1, w2, w3 = philox((i, born[:, None], generation, EM.W1_DOMAIN + k), key)
            y = x1 + (s_iso * EM.noise(w1, w2, w3))
            if s_line != 0:
                ak = a
                if variant == "a_per_element":
                    _, v1, v2, v3 = philox((i, born[:, None], generation, DOMAIN_A), key)
                    ak = s_line * EM.noise(v1, v2, v3)
                diff = (x1 - x2) if variant == "line_from_x2" else (x2 - x1)
                y = y + (ak * diff)
            assert y.dtype == f32
            kids[k].reshape(n_children, n)[born] = y
    return kids, parent, parent2, n_filled


def kid_bits(a):
    """float32 array -> uint32 words, every NaN mapped to one pattern: every element of a born child is computed, and a computed
    NaN has no defined sign or payload (evolve_model.bits says why)"""
    return EM.bits(a, np.ones(np.shape(a), bool))


# --------------------------------------------------------------------------------------------------------------- the forge
def forge(B, C, n_rows, seed=0):
    """-> (rows float32 [n_rows, B], centroids float32 [C, B]): small-integer-valued random rows and centroids (every operation
    exact: ties are real ties) with, as far as B, C and n_rows leave room, in this order: duplicate centroids; rows equal to a
    centroid, one of them with -0 against +0; rows half way between two centroids (an exact two-way tie) and at the centre of three
    (a three-way tie); rows with a NaN, +inf, -inf word; rows and a centroid at +-3e38 (the difference overflows); denormal rows and
    a denormal centroid; a NaN centroid.  The later half of the rows is inexact (4 N(0, 1)), so that every rounding of the sum shows
    in dist.  ``forge_facts`` says what a forged set really holds."""
    rng = np.random.default_rng([B, C, n_rows, seed])
    cen = rng.integers(-8, 9, (C, B)).astype(f32)
    rows = rng.integers(-8, 9, (n_rows, B)).astype(f32)
    if C >= 2:
        cen[1] = cen[0]                                        # a duplicate: it never wins
    if C >= 5:
        cen[2] = 0                                             # three centroids at the same distance from the origin's neighbour:
        cen[3] = 0                                             # cen[2] = (0, ..), cen[3] = (4, ..), cen[4] = (2, +-2 ..) around row (2, 0 ..)
        cen[4] = 0
        cen[3, 0] = 4
        cen[4, 0] = 2
        if B >= 2:
            cen[4, 1] = 2
    if C >= 7:
        cen[5] = f32(3e38)
        cen[6] = f32(1e-45) * rng.integers(1, 5, B).astype(f32)
    if C >= 9:
        cen[7, rng.integers(0, B)] = nan
        cen[8] = cen[0] + 16                                   # far from everything else, two apart from cen[9]: a clean two-way tie
    if C >= 10:
        cen[9] = cen[8]
        cen[9, 0] += 2
    r = 0

    def put(v):
        nonlocal r
        if r < n_rows:
            rows[r] = v
            r += 1
    put(cen[0])                                                # equal to a centroid (and to its duplicate)
    z = cen[0].copy()
    z[z == 0] = f32(-0.0)
    put(z)
    if C >= 5:
        mid = np.zeros(B, f32)
        mid[0] = 2
        put(mid)                                               # 4 from cen[2] and cen[3]; with B >= 2 also from cen[4]: a 2- or 3-way tie
        put(-0.0 * np.ones(B, f32))                            # -0 against the +0 centroid cen[2]
    if C >= 10:
        t = cen[8].copy()
        t[0] += 1
        put(t)                                                 # 1 from cen[8] and cen[9]
    for bad in (nan, inf, -inf):
        v = rng.integers(-8, 9, B).astype(f32)
        v[rng.integers(0, B)] = bad
        put(v)
    put(np.full(B, f32(-3e38)))                                # against cen[5]: 6e38 overflows; against the others t * t does
    put(np.full(B, f32(3e38)))
    put(f32(1e-45) * rng.integers(1, 9, B).astype(f32))        # denormals: t * t underflows to +0
    put(f32(1e-40) * np.ones(B, f32))
    half = max(r, n_rows // 2)                                 # the later half: inexact words, so that every rounding shows in dist
    rows[half:] = (rng.standard_normal((n_rows - half, B)) * 4.0).astype(f32)
    return rows, cen


def forge_facts(rows, cen):
    """what a forged set holds, from the model alone: counts of rows with an exact tie between two / among three and more centroids
    at the minimum, duplicate centroids, rows with distance 0 (and with a -0 word against a +0 one among them), rows with a NaN /
    an inf word, NaN centroids, rows whose every finite-looking difference overflows somewhere, denormal words, rows without a cell"""
    d2 = d2_model(rows, cen)
    cell, dist = assign_model(rows, cen)
    fin = np.where(np.isfinite(d2), d2, inf)
    at_min = (fin == dist[:, None]) & (dist[:, None] < inf)
    ties = at_min.sum(axis=1)
    dup = sum(1 for q in range(1, len(cen)) if any(np.array_equal(cen[q], cen[p]) for p in range(q)))
    zero = dist == 0
    minus = [bool(zero[r] and cell[r] >= 0 and (np.signbit(rows[r]) != np.signbit(cen[cell[r]])).any()) for r in range(len(rows))]
    finite_rows = np.isfinite(rows).all(axis=1)
    return dict(tie2=int((ties == 2).sum()), tie3=int((ties >= 3).sum()), duplicates=dup, equal=int(zero.sum()), minus_zero=int(sum(minus)),
                nan_rows=int(np.isnan(rows).any(axis=1).sum()), inf_rows=int(np.isinf(rows).any(axis=1).sum()),
                nan_centroids=int(np.isnan(cen).any(axis=1).sum()),
                overflow=int((finite_rows[:, None] & np.isfinite(cen).all(axis=1)[None, :] & ~np.isfinite(d2)).sum()),
                denormal=int(((rows != 0) & (np.abs(rows) < f32(1.2e-38))).sum() + ((cen != 0) & (np.abs(cen) < f32(1.2e-38))).sum()),
                no_cell=int((cell < 0).sum()))
