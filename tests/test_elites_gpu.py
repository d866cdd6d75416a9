"""MAP-Elites for device policies on a real MI355X (pytest -m gpu): rem2d_elites_insert / _sample / _emit against
tests/elites_model.py, every comparison by bits under `==` (NaNs at mutated elements mapped to one pattern), every buffer between
guard words, every input verified unchanged, every case run twice alike; the three builds; emit tied to rem2d_policy_vary bit for
bit; elites.EliteGrid, and two generations of evaluate.run_policy_map_elites against the host replay (the oracle's closed loop for
the episodes and the positions, elites_model for the rest).

Shapes: widths 1, 2, 8, 32; grids of 1, 2 and 4 dimensions with 1, 2, 63, 64, 65 and 1000 cells (65 536 at the smallest policy
shape); blocks below, at and above the wavefront and the 256-row tile (1, 2, 63, 64, 65, 257); one and three blocks; the smallest
policy shape (17 words per set: the one-word walk) and the workload's (MB 16, R 10, H 32) at aligned and 4-byte-offset bases, so
that the 16-byte and the one-word walk both run."""
import ctypes as C

import numpy as np
import pytest

import control_model as CM
import elites_model as QM
import evolve_model as EM
import novelty_model as NM
import policy_model as PM
from replay import need_gpu

pytestmark = pytest.mark.gpu

CONT = 1
f32, f64 = np.float32, np.float64
nan, inf = np.nan, np.inf
BUILDS = (False, True, "fma", False)                       # (the default build twice: each case runs twice alike)
GUARD = 16
WIDTHS = (1, 2, 8, 32)
SIZES = (1, 2, 63, 64, 65, 257)
BINS = {1: ([1], [1, 1], [1, 1, 1, 1]), 2: ([2], [2, 1], [1, 2, 1, 1]), 63: ([63], [9, 7], [3, 3, 7, 1]), 64: ([64], [8, 8], [4, 2, 4, 2]),
        65: ([65], [5, 13], [5, 1, 13, 1]), 1000: ([1000], [40, 25], [10, 5, 5, 4]), 65536: ([65536], [256, 256], [16, 16, 16, 16])}
CELLS = (1, 2, 63, 64, 65, 1000)
SMALL = ((14, 1), (1,), (1, 1), (1,))                      # MB 1, R 0, H 1
WORK = ((114, 32), (32,), (32, 16), (16,))                 # MB 16, R 10, H 32
ROWS = ("random", "one_cell", "own_cell", "special")
GRIDS = ("empty", "partly", "full")
NAMES = ("w1", "b1", "w2", "b2")


@pytest.fixture(scope="module")
def gpu():
    return need_gpu()


# ----------------------------------------------------------------------------------------------------------------- buffers
class Buf:
    """A device array between guard words, at an aligned or a 4-byte-offset base (float32 arrays; other types stay aligned)"""

    def __init__(self, torch, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        self.shape, self.dtype = arr.shape, arr.dtype
        self.n, self.at = arr.size, GUARD + (int(offset) if arr.dtype == np.float32 else 0)
        flat = np.full(self.n + 2 * GUARD + 1, 0, arr.dtype)
        flat[:] = self.pattern(len(flat))
        flat[self.at:self.at + self.n] = arr.ravel()
        self.host = flat.copy()
        self.t = torch.from_numpy(flat).to("cuda")

    def pattern(self, n):
        if self.dtype == np.float32:
            return np.full(n, 0xFFC0DE77, np.uint32).view(f32)       # (a NaN with a payload: == on bits)
        if self.dtype == np.float64:
            return np.full(n, 0xFFF8C0DE000000AA, np.uint64).view(f64)
        return np.full(n, 0x5A, self.dtype)

    @property
    def ptr(self):
        return self.t.data_ptr() + self.at * self.dtype.itemsize

    def read(self):
        """the array; the guards must be as they were"""
        flat = self.t.cpu().numpy()
        raw, was = flat.view(np.uint8), self.host.view(np.uint8)
        i0, i1 = self.at * self.dtype.itemsize, (self.at + self.n) * self.dtype.itemsize
        assert np.array_equal(raw[:i0], was[:i0]) and np.array_equal(raw[i1:], was[i1:]), "guard words were written"
        return flat[self.at:self.at + self.n].reshape(self.shape).copy()

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy().view(np.uint8), self.host.view(np.uint8))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_map(B, bins, rng):
    """a cell map with these bins over width B: distinct words where B allows, ranges of several scales"""
    n = len(bins)
    word = rng.permutation(B)[:n].tolist() if B >= n else [int(rng.integers(0, B)) for _ in range(n)]
    dims = []
    for i in range(n):
        lo = float(f32(rng.choice([-2.0, 0.0, -0.3, 1.0e3, -1.0e-3])))
        span = float(f32(rng.choice([4.0, 1.0, 0.7, 3.0e3, 2.0e-3])))
        dims.append((word[i], lo, float(f32(lo) + f32(span)), bins[i]))
    return QM.CellMap.of(dims), dims


def make_rows(kind, cmap, dims, M, S, B, rng):
    """desc float32 [M S, B] and fitness float64 [M S]"""
    G = M * S
    desc = rng.standard_normal((G, B)).astype(f32)
    fitness = rng.integers(-1, 3, G).astype(f64)                               # a coarse grid: ties
    fitness = np.where(rng.random(G) < 0.3, rng.standard_normal(G), fitness)
    special_f = np.array([0.0, -0.0, inf, -inf, nan, 5e-324, -5e-324, 2.2e-308], f64)
    hit = rng.random(G) < (0.5 if kind == "special" else 0.15)
    fitness[hit] = rng.choice(special_f, int(hit.sum()))
    for i, (w, lo, hi, n) in enumerate(dims):
        lo32, hi32 = f32(lo), f32(hi)
        if kind == "one_cell":
            desc[:, w] = lo32 + (hi32 - lo32) * f32(0.3)
            continue
        if kind == "own_cell":                                                 # row j of a block in cell j % C, at the cell's middle
            stride = int(np.prod(cmap.bins[:i], dtype=np.int64))
            q = (np.arange(G) % S % cmap.n_cells) // stride % n
            desc[:, w] = (lo32 + (q.astype(f32) + f32(0.5)) / cmap.inv[i]).astype(f32)
            continue
        x = (lo32 + (hi32 - lo32) * rng.random(G).astype(f32)).astype(f32)
        edge = (lo32 + rng.integers(0, n + 1, G).astype(f32) / cmap.inv[i]).astype(f32)    # lo, the interior edges, hi (or next to them)
        pick = rng.random(G)
        x = np.where(pick < 0.25, edge, x)
        x = np.where((pick >= 0.25) & (pick < 0.3), lo32, x)
        x = np.where((pick >= 0.3) & (pick < 0.35), hi32, x)
        x = np.where((pick >= 0.35) & (pick < 0.4), hi32 + (hi32 - lo32), x)
        x = np.where((pick >= 0.4) & (pick < 0.45), lo32 - (hi32 - lo32), x)
        if kind == "special":
            pool = np.array([nan, inf, -inf, 1e19, -1e19, 3e38, -3e38, 1e-45, -0.0], f32)
            sp = rng.random(G) < 0.3
            x = np.where(sp, rng.choice(pool, G), x)
        desc[:, w] = x.astype(f32)
    return desc, fitness


def make_grid(kind, M, C, B, shapes, rng):
    g = QM.Grid(M, C, B, shapes)
    g.desc[:] = rng.standard_normal(g.desc.shape)
    for w in g.weights:
        w[:] = rng.standard_normal(w.shape)
    g.fitness[:] = rng.standard_normal(g.fitness.shape)       # (what an empty cell holds means nothing and must stay)
    if kind == "empty":
        return g
    filled = rng.random((M, C)) < (0.5 if kind == "partly" else 2.0)
    g.count[:] = np.where(filled, rng.integers(1, 4, (M, C)), 0)
    # incumbents lower than, equal to and higher than the challengers' coarse grid, both zeros, the infinities, a NaN
    pool = np.array([-inf, -3.0, -1.0, -0.0, 0.0, 1.0, 2.0, 5e-324, 7.0, inf, nan], f64)
    g.fitness[:] = np.where(rng.random((M, C)) < 0.8, rng.choice(pool, (M, C)), g.fitness)
    return g


def descriptor(shapes, B, M, cmap, bufs, S=0, n_children=0, generation=0, seed=0, threshold=0, sigma=0.0):
    from gym_rem2d_amd import _lib
    e = _lib.Elites()
    e.d, e.hidden, e.max_bodies = shapes[0][0], shapes[0][1], shapes[3][0]
    e.width, e.n_blocks, e.group_size, e.n_children, e.n_dims = B, M, S, n_children, cmap.n_dims
    for i in range(cmap.n_dims):
        e.word[i], e.bins[i], e.lo[i], e.inv[i] = cmap.word[i], cmap.bins[i], cmap.lo[i], cmap.inv[i]
    e.generation, e.sigma, e.rate_threshold, e.seed, e.reserved = generation, sigma, threshold, seed, 0
    for k, b in bufs.items():
        setattr(e, k, b.ptr)
    e.scratch_bytes = 12 * M * cmap.n_cells
    return e


def call(torch, wide, name, e):
    from gym_rem2d_amd import _lib
    _lib.check(getattr(_lib.lib(wide), name)(C.byref(e), None), wide)
    torch.cuda.synchronize()


def grid_bufs(torch, g, offset, rng):
    """the grid's buffers, winner and a scratch full of garbage"""
    slots = g.M * g.C
    out = dict(elite_fitness=Buf(torch, g.fitness), elite_desc=Buf(torch, g.desc, offset), count=Buf(torch, g.count),
               winner=Buf(torch, np.full((g.M, g.C), 77, np.int32)),
               scratch=Buf(torch, rng.integers(-2 ** 62, 2 ** 62, (12 * slots + 7) // 8, dtype=np.int64)))
    for k, name in enumerate(NAMES):
        out["elite_" + name] = Buf(torch, g.weights[k], offset)
    return out


def same_grid(bufs, want, what):
    assert np.array_equal(bits(bufs["elite_fitness"].read()), bits(want.fitness)), what + ": elite_fitness"
    assert np.array_equal(bufs["count"].read(), want.count), what + ": count"
    assert np.array_equal(bits(bufs["elite_desc"].read()), bits(want.desc)), what + ": elite_desc"
    for k, name in enumerate(NAMES):
        assert np.array_equal(bits(bufs["elite_" + name].read()), bits(want.weights[k])), what + ": elite_" + name


def host_case(B, bins, S, M, shapes, rows, start, masked, off_grid, off_pop, S2, tag):
    """the host half of a case: two populations, the grid before and after each, the draw from the result, and what the case shows"""
    rng = np.random.default_rng([B, S, M, len(bins), int(np.prod(bins)), tag])
    cmap, dims = make_map(B, bins, rng)
    C_, G = cmap.n_cells, M * S
    grid0 = make_grid(start, M, C_, B, shapes, rng)
    pops, wants, g = [], [], grid0
    for rnd in range(2):
        desc, fitness = make_rows(rows if rnd == 0 else "random", cmap, dims, M, S, B, rng)
        weights = [rng.standard_normal((G,) + s).astype(f32) for s in shapes]
        weights[0][rng.random(weights[0].shape) < 0.01] = f32(nan)             # (a bit copy: payloads and all)
        mask = (rng.random(G) < 0.7).astype(np.uint8) if masked else None
        g, cell, winner = QM.insert_model(cmap, g, weights, fitness, desc, S, mask)
        pops.append((desc, fitness, weights, mask))
        wants.append((g, cell, winner))
    n_children = M * S2
    gen, seed = 3 + tag, (1 << 40) + 5 * tag
    n_filled, parent = QM.sample_model(g.count, n_children, seed, gen)
    cell1, win1 = wants[0][1], wants[0][2]
    ok = cell1 >= 0
    block = np.arange(G) // S
    cand = np.zeros((M, C_), bool)
    cand[block[ok], cell1[ok]] = True
    pairs = set(zip(block[ok].tolist(), cell1[ok].tolist()))
    saw = dict(one_cell=ok.sum() > 1 and len(set(cell1[ok].tolist())) == 1, own_cell=ok.sum() > 1 and len(pairs) == ok.sum(),
               held=int((cand & (win1 < 0)).sum()), replaced=int((win1 >= 0).sum()), second=int((wants[1][2] >= 0).sum()),
               dropped=int((~ok).sum()), empty_blocks=int((n_filled == 0).sum()))
    what = "B %d bins %s S %d M %d %s rows, %s grid, mask %s, offsets %d/%d" % (B, bins, S, M, rows, start, masked, off_grid, off_pop)
    return dict(cmap=cmap, grid0=grid0, pops=pops, wants=wants, n_children=n_children, gen=gen, seed=seed, n_filled=n_filled, parent=parent,
                saw=saw, what=what, rng=rng)


def insert_case(torch, B, bins, S, M, shapes, rows, start, masked, off_grid, off_pop, S2, tag, builds=BUILDS):
    """two inserts on top of each other and a sample of the result, in every build -> what the case saw"""
    H = host_case(B, bins, S, M, shapes, rows, start, masked, off_grid, off_pop, S2, tag)
    cmap, grid0, pops, wants, n_children, gen, seed, what, rng = (H[k] for k in ("cmap", "grid0", "pops", "wants", "n_children", "gen", "seed", "what", "rng"))
    G = M * S
    for wide in builds:
        gb = grid_bufs(torch, grid0, off_grid, rng)
        for rnd, ((desc, fitness, weights, mask), (want, cell, winner)) in enumerate(zip(pops, wants)):
            pb = dict(desc=Buf(torch, desc, off_pop), fitness=Buf(torch, fitness), cell=Buf(torch, np.full(G, 99, np.int32)))
            for k, name in enumerate(NAMES):
                pb[name] = Buf(torch, weights[k], off_pop)
            if mask is not None:
                pb["mask"] = Buf(torch, mask)
            call(torch, wide, "rem2d_elites_insert", descriptor(shapes, B, M, cmap, dict(gb, **pb), S=S))
            w = "%s, build %s, insert %d" % (what, wide, rnd + 1)
            assert np.array_equal(pb["cell"].read(), cell), w + ": cell"
            assert np.array_equal(gb["winner"].read(), winner), w + ": winner"
            same_grid(gb, want, w)
            assert all(pb[k].unchanged() for k in pb if k != "cell"), w + ": an input was written"
        gb["scratch"].read()                                                    # (its guards)
        sb = dict(count=gb["count"], scratch=gb["scratch"], parent=Buf(torch, np.full(n_children, 55, np.int32)),
                  n_filled=Buf(torch, np.full(M, 55, np.int32)))
        call(torch, wide, "rem2d_elites_sample", descriptor(shapes, B, M, cmap, sb, n_children=n_children, generation=gen, seed=seed))
        assert np.array_equal(sb["n_filled"].read(), H["n_filled"]), "%s, build %s: n_filled" % (what, wide)
        assert np.array_equal(sb["parent"].read(), H["parent"]), "%s, build %s: parent" % (what, wide)
        same_grid(gb, wants[1][0], "%s, build %s, after sample" % (what, wide))
    return H["saw"]


def cases_for(B):
    """(bins, S, M, shapes, rows, start, masked, off_grid, off_pop, S'): every S twice with this width; every cell count, both M, the three
    dimension counts, row and grid kinds, masks and bases in rotation.  The workload's shape where the grid is small"""
    out, i = [], WIDTHS.index(B)
    for s, S in enumerate(SIZES):
        for rep in range(2):
            t = 2 * s + rep + i
            C_ = CELLS[(s + 3 * rep + i) % 6]
            bins = BINS[C_][(s + rep + i) % 3]
            work = C_ <= 65 and (s + rep) % 2 == 0
            out.append((bins, S, (1, 3)[(s + rep + i) % 2], WORK if work else SMALL, ROWS[t % 4], GRIDS[(s + rep) % 3], t % 2 == 1,
                        (t // 2) % 2, (t // 3) % 2, (1, 64, 65)[t % 3]))
    return out


# --------------------------------------------------------------------------------------------------------- insert and sample
@pytest.mark.parametrize("B", WIDTHS)
def test_insert_and_sample(gpu, B):
    """rem2d_elites_insert (twice, the second on top of the first) and rem2d_elites_sample == elites_model, bit for bit, in the
    three builds, twice alike"""
    torch = gpu
    seen = {}
    for ci, case in enumerate(cases_for(B)):
        for k, v in insert_case(torch, B, *case[:9], S2=case[9], tag=ci).items():
            seen[k] = seen.get(k, 0) + int(v)
    print("B = %d: %d cases x 3 builds (one twice): %s" % (B, ci + 1, seen))
    assert seen["one_cell"] >= 1 and seen["own_cell"] >= 1 and seen["held"] >= 1 and seen["replaced"] >= 1 and seen["second"] >= 1 and seen["dropped"] >= 1


def test_the_largest_grid(gpu):
    """65 536 cells at the smallest policy shape, in 1, 2 and 4 dimensions; every row in a cell of its own among them"""
    torch = gpu
    for n, (S, M, rows) in enumerate(((257, 1, "own_cell"), (65, 3, "random"), (64, 1, "special"))):
        got = insert_case(torch, (2, 8, 32)[n], BINS[65536][n], S, M, SMALL, rows, GRIDS[n], n == 1, 0, n % 2, S2=(65, 1, 64)[n], tag=100 + n, builds=(False, True, "fma"))
        assert got["replaced"] >= 1 and got["second"] >= 1


# -------------------------------------------------------------------------------------------------------------------- emit
def emit_grid(C_, shapes, rng):
    """three blocks: no filled cell, one, all"""
    g = make_grid("empty", 3, C_, 2, shapes, rng)
    g.count[1, C_ // 2] = 2
    g.count[2] = rng.integers(1, 4, C_)
    g.weights[0][rng.random(g.weights[0].shape) < 0.01] = f32(nan)
    g.weights[2][2 * C_, 0, 0], g.weights[3][-1, 0] = f32(-0.0), f32(inf)
    return g


@pytest.mark.parametrize("shape", ["small", "work"])
def test_emit(gpu, shape):
    """rem2d_elites_emit == elites_model.emit_model == rem2d_policy_vary from the flattened elite arrays and the same parents: blocks
    with 0, 1 and C filled cells, 1, 64 and 65 children per block, rates 0, 0.3 and 1, aligned and offset bases; the children of the
    empty block keep their sentinels; the grid is not written"""
    torch = gpu
    from gym_rem2d_amd import _lib
    shapes, C_ = (SMALL, 65) if shape == "small" else (WORK, 5)
    cmap = QM.CellMap([0], [C_], [0.0], [1.0])
    for ci, (S2, rate, off_grid, off_kid) in enumerate(((1, 0.3, 0, 0), (64, 1.0, 0, 0), (65, 0.0, 0, 0), (65, 0.3, 1, 0), (64, 0.3, 0, 1), (65, 1.0, 1, 1))):
        rng = np.random.default_rng([C_, S2, ci])
        g = emit_grid(C_, shapes, rng)
        n, thr, sigma, seed, gen = 3 * S2, EM.rate_threshold(rate), 0.25, (7 << 33) + ci, 11 + ci
        sentinel = [rng.standard_normal((n,) + s).astype(f32) for s in shapes]
        kids, hits, parent, n_filled = QM.emit_model(g, n, thr, sigma, seed, gen, before=sentinel)
        assert n_filled.tolist() == [0, 1, C_] and (parent[:S2] == -1).all() and (parent[S2:2 * S2] == C_ + C_ // 2).all()
        assert S2 == 1 or len(set(parent[2 * S2:].tolist())) > 1
        assert all(np.array_equal(bits(kids[k][:S2]), bits(sentinel[k][:S2])) for k in range(4))
        share = sum(int(h[S2:].sum()) for h in hits) / float(sum(h[S2:].size for h in hits))
        assert (rate == 0.0 and share == 0) or (rate == 1.0 and share == 1) or (rate == 0.3 and (S2 == 1 or 0.25 < share < 0.35))
        what = "%s shape, S' %d, rate %s, offsets %d/%d" % (shape, S2, rate, off_grid, off_kid)
        for wide in BUILDS:
            gb = grid_bufs(torch, g, off_grid, rng)
            eb = dict(parent=Buf(torch, np.full(n, 55, np.int32)), n_filled=Buf(torch, np.full(3, 55, np.int32)))
            for k, name in enumerate(NAMES):
                eb["child_" + name] = Buf(torch, sentinel[k], off_kid)
            bufs = {k: v for k, v in dict(gb, **eb).items() if k not in ("winner", "elite_fitness", "elite_desc")}
            e = descriptor(shapes, 2, 3, cmap, bufs, n_children=n, generation=gen, seed=seed, threshold=thr, sigma=sigma)
            call(torch, wide, "rem2d_elites_emit", e)
            assert np.array_equal(eb["parent"].read(), parent) and np.array_equal(eb["n_filled"].read(), n_filled), what
            got = [eb["child_" + name].read() for name in NAMES]
            for k, name in enumerate(NAMES):
                assert np.array_equal(EM.bits(got[k], hits[k]), EM.bits(kids[k], hits[k])), "%s, build %s: child_%s" % (what, wide, name)
            same_grid(gb, g, what + ": the grid after emit")
            # the older operator, from the same arrays and parents: N = max(M C, M S') sets on both sides, the rest without a parent
            N = max(3 * C_, n)
            vb = dict(parent=Buf(torch, np.concatenate([parent, np.full(N - n, -1, np.int32)])))
            v = _lib.Evolve()
            v.d, v.hidden, v.max_bodies, v.n_sets, v.group_size = shapes[0][0], shapes[0][1], shapes[3][0], N, N
            v.tournsize, v.elite, v.generation, v.rate_threshold, v.seed, v.sigma, v.reserved = 1, 0, gen, thr, seed, sigma, 0
            for k, name in enumerate(NAMES):
                src = np.concatenate([g.weights[k], np.zeros((N - 3 * C_,) + shapes[k], f32)])
                dst = np.concatenate([sentinel[k], np.zeros((N - n,) + shapes[k], f32)])
                vb[name], vb["child_" + name] = Buf(torch, src, off_grid), Buf(torch, dst, off_kid)
                setattr(v, name, vb[name].ptr)
                setattr(v, "child_" + name, vb["child_" + name].ptr)
            v.parent = vb["parent"].ptr
            _lib.check(_lib.lib(wide).rem2d_policy_vary(C.byref(v), None), wide)
            torch.cuda.synchronize()
            for k, name in enumerate(NAMES):
                old = vb["child_" + name].read()
                assert np.array_equal(bits(old[:n]), bits(got[k])), "%s, build %s: child_%s differs from rem2d_policy_vary's" % (what, wide, name)
                assert (old[n:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- EliteGrid
def test_elite_grid(gpu):
    """elites.EliteGrid: insert / sample / emit give the model's bits, out= is written in place and nothing else is allocated, the
    readings, a checkpoint restores the grid"""
    torch = gpu
    from gym_rem2d_amd import elites, policy
    M, S, B = 2, 64, 4
    dims = [(1, -2.0, 2.0, 6), (3, -1.0, 3.0, 5)]
    cmap = QM.CellMap.of(dims)
    rng = np.random.default_rng(31)
    like = policy.MLPPolicy.random(M * S, 16, 32).to("cuda")
    grid = elites.EliteGrid(M, dims, B, like=like, device="cuda")
    assert np.array_equal(np.array(grid.inv, f32), np.array(cmap.inv, f32)) and grid.n_cells == 30
    model = QM.Grid(M, 30, B, WORK)
    kids = policy.MLPPolicy.random(M * S, 16, 32, seed=1).to("cuda")
    mem, partly = [], 0
    pop = like
    for gen in range(1, 5):
        desc = (rng.standard_normal((M * S, B)) * 1.5).astype(f32)
        fit = rng.integers(0, 4, M * S).astype(f64)
        if gen == 1:
            desc[S:] = nan                                                     # block 1 stays empty for a generation
        weights = [t.cpu().numpy() for t in (pop.w1, pop.b1, pop.w2, pop.b2)]
        winner = grid.insert(pop, torch.from_numpy(fit).to("cuda"), torch.from_numpy(desc).to("cuda"))
        model, cell, want_winner = QM.insert_model(cmap, model, weights, fit, desc, S)
        assert winner is grid.winner and np.array_equal(winner.cpu().numpy(), want_winner) and np.array_equal(grid.cell.cpu().numpy(), cell)
        assert np.array_equal(bits(grid.fitness.cpu().numpy()), bits(model.fitness)) and np.array_equal(grid.count.cpu().numpy(), model.count)
        assert np.array_equal(bits(grid.desc.cpu().numpy()), bits(model.desc))
        for k, t in enumerate((grid.w1, grid.b1, grid.w2, grid.b2)):
            assert np.array_equal(bits(t.cpu().numpy()), bits(model.weights[k])), "generation %d, %s" % (gen, NAMES[k])
        filled = model.count != 0
        partly += int(((filled.sum(axis=1) > 1) & (filled.sum(axis=1) < 30)).sum())
        assert grid.n_filled.cpu().tolist() == filled.sum(axis=1).tolist() and (gen > 1 or grid.n_filled.cpu().tolist()[1] == 0)
        assert np.array_equal(grid.coverage().cpu().numpy(), filled.sum(axis=1) / 30.0)
        assert np.allclose(grid.qd_score().cpu().numpy(), np.where(filled, model.fitness, 0).sum(axis=1), rtol=1e-12)
        before = [t.cpu().numpy() for t in (kids.w1, kids.b1, kids.w2, kids.b2)]
        out = grid.emit(gen, seed=9, rate=0.3, sigma=0.2, out=kids, wide=(False, True, "fma", False)[gen - 1])
        assert out is kids
        want, hits, parent, n_filled = QM.emit_model(model, M * S, EM.rate_threshold(0.3), 0.2, 9, gen, before=before)
        assert np.array_equal(kids.parents.cpu().numpy(), parent) and np.array_equal(grid.filled.cpu().numpy(), n_filled)
        for k, t in enumerate((kids.w1, kids.b1, kids.w2, kids.b2)):
            assert np.array_equal(EM.bits(t.cpu().numpy(), hits[k]), EM.bits(want[k], hits[k])), "generation %d, child %s" % (gen, NAMES[k])
        assert np.array_equal(grid.sample(gen, seed=9, n_children=M * S).cpu().numpy(), parent)
        pop = kids
        torch.cuda.synchronize()
        mem.append(torch.cuda.memory_allocated())
    assert mem[2] == mem[1] == mem[3], mem
    assert (model.count > 1).any() and partly >= 1                           # (the draws saw grids that were neither empty nor full)
    best = grid.elites(1)
    rows = np.flatnonzero(model.count[1] != 0) + 30
    assert best.n_sets == len(rows) and np.array_equal(bits(best.w1.cpu().numpy()), bits(model.weights[0][rows]))
    fresh = grid.emit(7, n_children=M * 3)
    assert fresh.n_sets == 6 and fresh.parents.shape == (6,) and (fresh.parents.cpu().numpy() >= 0).all()
    state = grid.state_dict()
    other = elites.EliteGrid(M, dims, B, like=like, device="cuda")
    other.load_state_dict(state)
    grid.count.zero_()
    assert np.array_equal(other.count.cpu().numpy(), model.count) and np.array_equal(other.sample(5, n_children=M * S).cpu().numpy(), QM.sample_model(model.count, M * S, 0, 5)[1])
    assert (grid.sample(5, n_children=M * S).cpu().numpy() == -1).all()


# ------------------------------------------------------------------------------------------------------------- generations
def behaviour_replay(O, terrain, morphs, rows, weights, flags, n_steps, max_bodies, period, samples):
    """evolve_model.episode_replay that also describes: the oracle's closed loop under the weight sets, from reset, with
    describe_update at step 0 and after every `period` steps -> (fitness float64 [n], behaviour float32 [n, 2 samples], gone)"""
    import range_model as R
    T = R.Terrain.of(terrain)
    rays = R.bipedal_rays()
    n = sum(len(r) for r in rows)
    fitness, gone, beh = np.zeros(n, f64), np.zeros(n, bool), np.zeros((n, 2 * samples), f32)
    for morph, r in zip(morphs, rows):
        loop = CM.OracleLoop(O, terrain, morph, flags, "replay")
        ctx = loop.ctx
        W = [a[np.asarray(r)] for a in weights]
        run = dict(ctx=ctx, caps=[], obs=[])
        mine = np.zeros((ctx.N, 2 * samples), f32)
        for t in range(n_steps + 1):
            snap = loop.snapshot()
            run["obs"].append(None)
            run["caps"].append(np.stack([snap["ccount"].max(axis=1),
                                         ((snap["ctouch"] != 0) & CM.F.masks(ctx, snap)["cedge"]).sum(axis=0).max(axis=1)], 1))
            if t % period == 0 and t <= period * samples:
                NM.describe_update(mine, loop.env["steps"], loop.env["frozen"], snap["px"][:, 0], snap["py"][:, 0], period, samples)
            if t == n_steps:
                break
            obs = CM.observe_model(ctx, snap, max_bodies)
            frac = R.cast(T, snap["px"][:, 0], snap["py"][:, 0], rays)[0]
            tg, valid = PM.forward_model(PM.input_rows(obs, frac), *W)
            loop.set_targets(tg, mask=valid)
            loop.step()
        fitness[r], beh[r] = loop.env["fitness"], mine
        gone[r] = CM.left_out_first(run)[0] < len(run["obs"])
    return fitness, beh, gone


LOOP = dict(steps=60, S=16, K=4, period=15, rate=0.3, sigma=0.1, seed=7,
            dims=[(6, 3.0, 7.0, 8), (7, 5.2, 6.0, 4)])            # the root's last recorded x and y; some end beyond both ranges


def host_generations(oracle):
    """-> (batches, W, want): the population, generation 0's weight sets and the host's generations 0, 1 and 2"""
    from gym_rem2d_amd import make_terrain, synthetic
    from gym_rem2d_amd.compiler import Morphology, lanes_for
    specs = [s for s in synthetic.lsystem_specs(range(120)) if s.n_bodies >= 2][:64]
    n, steps, S, K, period = len(specs), LOOP["steps"], LOOP["S"], LOOP["K"], LOOP["period"]
    M = n // S
    groups = {}
    for e, s in enumerate(specs):
        groups.setdefault(lanes_for(s.n_bodies), []).append(e)
    batches = [(Morphology.from_specs([specs[e] for e in groups[g]], g), groups[g]) for g in sorted(groups)]
    morphs, rows = [m for m, _ in batches], [np.asarray(idx) for _, idx in batches]
    terrain = make_terrain(4)
    W = list(PM.loop_weights(n, 16))
    cmap = QM.CellMap.of(LOOP["dims"])
    grid = QM.Grid(M, cmap.n_cells, 2 * K, [a.shape[1:] for a in W])
    want, kids = [], W
    for gen in (0, 1, 2):
        parent = None
        if gen:
            kids, _, parent, _ = QM.emit_model(grid, n, EM.rate_threshold(LOOP["rate"]), LOOP["sigma"], LOOP["seed"], gen, before=kids)
        fit, beh, gone = behaviour_replay(oracle, terrain, morphs, rows, kids, CONT, steps, PM.LOOP_BODIES, period, K)
        assert not gone.any()
        grid, cell, winner = QM.insert_model(cmap, grid, kids, fit, beh, S)
        want.append(dict(kids=kids, fit=fit, beh=beh, grid=grid, cell=cell, winner=winner, parent=parent))
    # the replay is worth comparing with: several cells per block, replacements in the later generations, some that hold
    filled = (grid.count != 0).sum(axis=1)
    assert (filled >= 2).all() and (grid.count > 1).any() and all((w["winner"] >= 0).any() for w in want[1:])
    assert len(set(want[1]["parent"].tolist())) > M
    return batches, W, want


def test_two_generations_of_map_elites(gpu, oracle):
    """evaluate.run_policy_map_elites on 64 L-system creatures in blocks of 16, episodes of 60 steps described 4 times, an 8 x 4 grid
    over the root's last position: generation 0 and two more give the host replay's children, parents, fitness, behaviour, cells,
    winners and grid; the second generation allocates nothing; a checkpoint restores the grid"""
    torch = gpu
    from gym_rem2d_amd import elites, evaluate, policy
    from gym_rem2d_amd.env import BatchedModular2D
    batches, W, want = host_generations(oracle)
    n = sum(m.n_envs for m, _ in batches)
    steps, S, K, period = LOOP["steps"], LOOP["S"], LOOP["K"], LOOP["period"]
    env = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
    try:
        env.reset_batches(batches, n)
        first = policy.MLPPolicy(*[torch.from_numpy(a.copy()) for a in W]).to("cuda")
        grid = elites.EliteGrid(n // S, LOOP["dims"], 2 * K, like=first, device="cuda")
        seen, mem = [], []

        def keep(g, kids, f, b, gr):
            seen.append(dict(kids=[t.cpu().numpy() for t in (kids.w1, kids.b1, kids.w2, kids.b2)], fit=f.cpu().numpy(), beh=b.cpu().numpy(),
                             parent=None if g == 0 else kids.parents.cpu().numpy(), cell=gr.cell.cpu().numpy(), winner=gr.winner.cpu().numpy(),
                             state={k: v.cpu().numpy() for k, v in gr.state_dict().items()}))
            torch.cuda.synchronize()
            mem.append(torch.cuda.memory_allocated())
        got_grid, fit, history = evaluate.run_policy_map_elites(env, first, grid, 2, period=period, samples=K, seed=LOOP["seed"], rate=LOOP["rate"],
                                                                 sigma=LOOP["sigma"], group_size=S, max_steps=steps, on_generation=keep)
        assert got_grid is grid and len(seen) == 3 and [h[0] for h in history] == [0, 1, 2]
        for g, (got, w) in enumerate(zip(seen, want)):
            for k in range(4):
                assert np.array_equal(bits(got["kids"][k]), bits(w["kids"][k])), "generation %d: children, %s" % (g, NAMES[k])
            assert g == 0 or np.array_equal(got["parent"], w["parent"]), "generation %d: parents" % g
            assert np.array_equal(bits(got["fit"]), bits(w["fit"])), "generation %d: fitness" % g
            assert np.array_equal(bits(got["beh"]), bits(w["beh"])), "generation %d: behaviour" % g
            assert np.array_equal(got["cell"], w["cell"]) and np.array_equal(got["winner"], w["winner"]), "generation %d: cell, winner" % g
            m = w["grid"]
            for key, arr in (("fitness", m.fitness), ("desc", m.desc), ("count", m.count), ("w1", m.weights[0]), ("b1", m.weights[1]),
                             ("w2", m.weights[2]), ("b2", m.weights[3])):
                assert np.array_equal(bits(got["state"][key]), bits(arr)), "generation %d: the grid's %s" % (g, key)
            filled = m.count != 0
            assert history[g][4] == int(filled.sum()) and history[g][1] == w["fit"].min() and history[g][2] == w["fit"].max()
            assert abs(history[g][5] - np.where(filled, m.fitness, 0.0).sum()) < 1e-9
        assert np.array_equal(bits(fit.cpu().numpy()), bits(want[2]["fit"]))
        assert np.array_equal(bits(first.w1.cpu().numpy()), bits(W[0]))             # the caller's policy is never written
        assert mem[2] == mem[1], mem
        state = grid.state_dict()
        again = elites.EliteGrid(n // S, LOOP["dims"], 2 * K, like=first, device="cuda")
        again.load_state_dict(state)
        a, b = grid.emit(3, seed=1, n_children=n), again.emit(3, seed=1, n_children=n)
        assert np.array_equal(a.parents.cpu().numpy(), b.parents.cpu().numpy()) and np.array_equal(bits(a.w1.cpu().numpy()), bits(b.w1.cpu().numpy()))
    finally:
        env.close()
