"""MAP-Elites for device policies stated on the host (include/rem2d_elites.h), shared by tests/test_elites_host.py (numpy alone) and
tests/test_elites_gpu.py: what novelty_model.py is for the novelty score.  Written from the header, not from the kernels.

* ``CellMap``: the dimensions of a grid; ``CellMap.of`` computes ``inv`` as the Python layer does.
* ``cells_model``: cell int32 [G] of every row, -1 for a row that is not admissible.
* ``Grid``: the state the caller owns, as numpy arrays; ``insert_model`` files a population into it.
* ``sample_model``: (n_filled, parent); ``emit_model``: the children, through evolve_model's mutation.

The ``variant`` names state WRONG rules, for the teeth test of test_elites_host.py.
"""
import numpy as np

import evolve_model as EM
from evolve_model import philox, rate_threshold, seed_key  # noqa: F401  (rate_threshold: re-exported)

f32, f64 = np.float32, np.float64
u32, u64 = np.uint32, np.uint64
ELITES_DOMAIN = 10                                         # counter word 3 of the draw; 0 .. 4 evolve, 5 .. 8 the strategy, 9 novelty
MAX_CELLS = 65536
VARIANTS = ("high_ties", "replace_equal", "round", "reverse_strides", "drop_outside", "draw_all_cells", "minus_zero_below")


class CellMap:
    def __init__(self, word, bins, lo, inv):
        self.word, self.bins = [int(w) for w in word], [int(b) for b in bins]
        self.lo, self.inv = [f32(v) for v in lo], [f32(v) for v in inv]
        self.n_dims = len(self.word)
        self.n_cells = int(np.prod(self.bins, dtype=np.int64))
        assert 1 <= self.n_dims <= 4 and all(b >= 1 for b in self.bins) and self.n_cells <= MAX_CELLS
        assert all(np.isfinite(v) for v in self.lo) and all(np.isfinite(v) and v > 0 for v in self.inv)

    @classmethod
    def of(cls, dims):
        """dims [(word, lo, hi, bins)]: inv = float32(bins) / (float32(hi) - float32(lo)), in binary32"""
        inv = [f32(n) / (f32(h) - f32(l)) for _, l, h, n in dims]
        assert all(v.dtype == f32 for v in inv)
        return cls([d[0] for d in dims], [d[3] for d in dims], [d[1] for d in dims], inv)


def cells_model(cmap, desc, fitness, mask=None, variant=None):
    """cell int32 [G]: -1 for a row with a non-finite selected word, a NaN fitness or a cleared mask entry"""
    desc = np.asarray(desc, f32)
    G = desc.shape[0]
    ok = ~np.isnan(np.asarray(fitness, f64))
    if mask is not None:
        ok &= np.asarray(mask) != 0
    cell = np.zeros(G, np.int64)
    strides = np.cumprod([1] + cmap.bins[:-1])
    if variant == "reverse_strides":
        strides = np.cumprod([1] + cmap.bins[::-1][:-1])[::-1]
    for i in range(cmap.n_dims):
        x = desc[:, cmap.word[i]]
        ok &= np.isfinite(x)
        with np.errstate(all="ignore"):
            u = (x - cmap.lo[i]) * cmap.inv[i]              # two float32 operations
        assert u.dtype == f32
        nb = cmap.bins[i]
        fin = np.where(np.isfinite(u), u, f32(0))
        if variant == "round":
            q = np.rint(np.clip(fin.astype(f64), -1.0, float(nb))).astype(np.int64)
        else:
            q = np.trunc(np.clip(fin.astype(f64), -1.0, float(nb))).astype(np.int64)
        below, above = u < 0, u >= f32(nb)
        if variant == "drop_outside":
            ok &= ~(below | above)
        q = np.where(below, 0, np.where(above, nb - 1, np.clip(q, 0, nb - 1)))
        cell += q * int(strides[i])
    return np.where(ok, cell, -1).astype(np.int32)


class Grid:
    """elite_fitness [M, C], elite_desc [M, C, B], count [M, C] and the four weight arrays [M C, ...]"""

    def __init__(self, M, C, B, shapes):
        self.M, self.C, self.B = int(M), int(C), int(B)
        self.fitness = np.zeros((M, C), f64)
        self.desc = np.zeros((M, C, B), f32)
        self.count = np.zeros((M, C), np.int32)
        self.weights = [np.zeros((M * C,) + tuple(s), f32) for s in shapes]

    def copy(self):
        g = Grid.__new__(Grid)
        g.M, g.C, g.B = self.M, self.C, self.B
        g.fitness, g.desc, g.count = self.fitness.copy(), self.desc.copy(), self.count.copy()
        g.weights = [w.copy() for w in self.weights]
        return g

    def words(self):
        """every bit of the grid as one uint32 array (for == and for counting what changed)"""
        return np.concatenate([self.fitness.view(u32).ravel(), self.desc.view(u32).ravel(), self.count.view(u32).ravel()]
                              + [w.view(u32).ravel() for w in self.weights])


def insert_model(cmap, grid, weights, fitness, desc, group_size, mask=None, variant=None):
    """-> (grid after, cell int32 [G], winner int32 [M, C]); the inputs are not written"""
    assert variant is None or variant in VARIANTS
    fitness, desc = np.asarray(fitness, f64), np.asarray(desc, f32)
    G, S = fitness.shape[0], int(group_size)
    M, C = grid.M, grid.C
    assert G == M * S and C == cmap.n_cells
    cell = cells_model(cmap, desc, fitness, mask, variant)
    out = grid.copy()
    winner = np.full((M, C), -1, np.int32)

    def above(a, b):
        if variant == "minus_zero_below" and a == 0 and b == 0:
            return bool(np.signbit(b) and not np.signbit(a))
        return bool(EM.greater(a, b))
    for c in range(G):                                     # ascending rows: a tie keeps the earlier one
        q = cell[c]
        if q < 0:
            continue
        b = c // S
        w = winner[b, q]
        if w < 0 or above(fitness[c], fitness[w]) or (variant == "high_ties" and not above(fitness[w], fitness[c])):
            winner[b, q] = c
    for b in range(M):
        for q in range(C):
            w = winner[b, q]
            if w < 0:
                continue
            better = above(fitness[w], grid.fitness[b, q]) or (variant == "replace_equal" and not above(grid.fitness[b, q], fitness[w]))
            if grid.count[b, q] != 0 and not better:
                winner[b, q] = -1
                continue
            out.fitness[b, q] = fitness[w]
            out.desc[b, q] = desc[w]
            out.count[b, q] = grid.count[b, q] + 1
            for k in range(4):
                out.weights[k][b * C + q] = np.asarray(weights[k], f32)[w]
    return out, cell, winner


def sample_model(count, n_children, seed, generation, variant=None):
    """count int32 [M, C] -> (n_filled int32 [M], parent int32 [n_children])"""
    count = np.asarray(count)
    M, C = count.shape
    per = int(n_children) // M
    assert per * M == n_children and per >= 1
    c = np.arange(n_children, dtype=np.int64)
    x0 = philox((0, c, generation, ELITES_DOMAIN), seed_key(seed))[0].astype(u64)
    parent = np.full(n_children, -1, np.int32)
    n_filled = np.zeros(M, np.int32)
    for b in range(M):
        f = np.flatnonzero(count[b] != 0)
        n_filled[b] = len(f)
        if len(f) == 0:
            continue
        if variant == "draw_all_cells":
            f = np.arange(C)
        j = ((x0[b * per:(b + 1) * per] * u64(len(f))) >> u64(32)).astype(np.int64)
        parent[b * per:(b + 1) * per] = b * C + f[j]
    return n_filled, parent


def emit_model(grid, n_children, threshold, sigma, seed, generation, before=None, variant=None):
    """-> (children: four arrays [n_children, ...], hits, parent, n_filled).  A child whose parent is -1 keeps what ``before``
    (four arrays, default zeros) holds"""
    n_filled, parent = sample_model(grid.count, n_children, seed, generation, variant)
    kids = [np.zeros((n_children,) + a.shape[1:], f32) if before is None else np.array(before[k], f32) for k, a in enumerate(grid.weights)]
    hits = [np.zeros(a.shape, bool) for a in kids]
    born = np.flatnonzero(parent >= 0)
    for k, a in enumerate(grid.weights):                   # evolve_model.mutate_set for all born children of an array at once
        n = int(np.prod(a.shape[1:], dtype=np.int64))
        src = a.reshape(a.shape[0], n)[parent[born]]
        x0, x1, x2, x3 = philox((np.arange(n, dtype=np.int64)[None, :], born[:, None], generation, EM.W1_DOMAIN + k), seed_key(seed))
        hit = x0.astype(u64) < u64(int(threshold))
        with np.errstate(all="ignore"):
            moved = src + (f32(sigma) * EM.noise(x1, x2, x3))
        assert moved.dtype == f32
        kids[k].reshape(n_children, n)[born] = np.where(hit, moved, src)
        hits[k].reshape(n_children, n)[born] = hit
    return kids, hits, parent, n_filled


def bits64(a):
    """float64 array -> uint64 words (fitness values are copied, never computed: NaN payloads are compared too)"""
    return np.ascontiguousarray(a, f64).view(u64)
