"""Centroid archives and the iso+line emitter on a real MI355X (pytest -m gpu): rem2d_cvt_assign / _insert / _emit_line against
tests/cvt_model.py, every comparison by bits under `==` (computed NaNs mapped to one pattern), every buffer between guard words,
every input verified unchanged, in the three builds; every launch shape of the assignment the same bits; elites.CentroidArchive,
EliteGrid.emit_line tied to EliteGrid.emit, cvt_centroids on the GPU against the CPU, two generations of
evaluate.run_policy_map_elites over a centroid archive with the line emitter, the three calls under a capture and behind a gate on a
caller's stream, and the refusals.

Shapes: widths 1, 3, 8, 32 (every padded width) x 1, 2, 65, 257 centroids (below, at and above one LDS tile of 256) x 6, 201 and 515
rows (a partial wavefront, a partial workgroup, three workgroups); 65 536 centroids x 64 rows for the split; policy sets with 16-byte
and 4-byte arrays at aligned and 4-byte-offset bases."""
import ctypes as C

import numpy as np
import pytest

import cvt_model as VM
import elites_model as QM
import policy_model as PM
import test_caller_stream_gpu as TCS
import test_elites_gpu as TEL
from replay import need_gpu
from test_caller_stream_gpu import gate  # noqa: F401  (the fixture: the gate's cycle count, proved by its control)
from test_elites_gpu import Buf, bits

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
nan, inf = np.nan, np.inf
BUILDS = (False, True, "fma")
WIDTHS, CELLS, ROWS = (1, 3, 8, 32), (1, 2, 65, 257), (6, 201, 515)
MIXED = ((35, 5), (5,), (5, 4), (4,))                      # MB 4, R 3, H 5: per-set lengths 175 5 20 4 -- two 4-byte and two 16-byte arrays
WORK = TEL.WORK                                            # MB 16, R 10, H 32
NAMES = TEL.NAMES


@pytest.fixture(scope="module")
def gpu():
    return need_gpu()


@pytest.fixture(scope="module", autouse=True)
def _released():
    yield
    TCS._MEMO.clear()


def descriptor(bufs, shapes=MIXED, **kw):
    from gym_rem2d_amd import _lib
    v = _lib.Cvt()
    v.d, v.hidden, v.max_bodies = shapes[0][0], shapes[0][1], shapes[3][0]
    for k, b in bufs.items():
        setattr(v, k, b.ptr)
    v.scratch_bytes = getattr(bufs.get("scratch"), "n", 0) * 8
    for k, x in kw.items():
        setattr(v, k, x)
    return v


def call(torch, wide, name, v, expect=0):
    from gym_rem2d_amd import _lib
    rc = getattr(_lib.lib(wide), name)(C.byref(v))
    torch.cuda.synchronize()
    if expect == 0:
        _lib.check(rc, wide)
    else:
        assert rc == expect, (name, rc)
    return _lib.lib(wide).rem2d_last_error()


def scratch(torch, words, rng):
    return Buf(torch, rng.integers(-2 ** 62, 2 ** 62, max(int(words), 1), dtype=np.int64))


# ------------------------------------------------------------------------------------------------------------------ assign
def assign_case(torch, B, C_, n, wide, splits, offset, rng, cen=None, rows=None):
    if rows is None:
        rows, cen = VM.forge(B, C_, n)
    want = VM.assign_model(rows, cen)
    bufs = dict(desc=Buf(torch, rows, offset), centroids=Buf(torch, cen, offset), cell=Buf(torch, np.full(n, 99, np.int32)),
                dist=Buf(torch, np.full(n, 5.0, f32), offset), scratch=scratch(torch, n, rng))
    call(torch, wide, "rem2d_cvt_assign", descriptor(bufs, width=B, n_cells=C_, n_rows=n, splits=splits))
    what = "B %d C %d rows %d build %s splits %d offset %d" % (B, C_, n, wide, splits, offset)
    assert np.array_equal(bufs["cell"].read(), want[0]), what + ": cell"
    assert np.array_equal(bits(bufs["dist"].read()), bits(want[1])), what + ": dist"
    assert bufs["desc"].unchanged() and bufs["centroids"].unchanged(), what + ": an input was written"
    bufs["scratch"].read()
    return want


@pytest.mark.parametrize("B", WIDTHS)
def test_assign(gpu, B):
    """cell and dist == cvt_model.assign_model on the forge (ties, duplicates, +-0, NaN, +-inf, overflow, denormals), in the three
    builds, at aligned and odd 4-byte offsets, with the library's launch shape and with 1, 2, 3 and 5 splits; dist = NULL; the
    all-NaN table"""
    torch = gpu
    from gym_rem2d_amd import _lib
    rng = np.random.default_rng(B)
    no_cell = 0
    for C_ in CELLS:
        for n in ROWS:
            for i, wide in enumerate(BUILDS):
                for splits in (0, 1, 2, 3, 5):
                    want = assign_case(torch, B, C_, n, wide, splits, (i + splits + n) % 2, rng)
                    no_cell += int((want[0] < 0).sum())
        # no dist; the all-NaN table
        rows, cen = VM.forge(B, C_, 201)
        for splits in (1, 4):
            bufs = dict(desc=Buf(torch, rows, 1), centroids=Buf(torch, cen), cell=Buf(torch, np.full(201, 99, np.int32)), scratch=scratch(torch, 201, rng))
            call(torch, False, "rem2d_cvt_assign", descriptor(bufs, width=B, n_cells=C_, n_rows=201, splits=splits))
            assert np.array_equal(bufs["cell"].read(), VM.assign_model(rows, cen)[0])
            want = assign_case(torch, B, C_, 201, "fma", splits, 1, rng, cen=np.full_like(cen, nan), rows=rows)
            assert (want[0] == -1).all() and np.isposinf(want[1]).all()
    assert no_cell > 0
    assert _lib.lib(False).rem2d_cvt_abi_version() == 1


def test_assign_split_over_65536_centroids(gpu):
    """64 rows against 65 536 centroids of 8 words: the library splits the centroids over workgroups (clear, atomicMin of
    (d2 bits, q), read-out); the same bits as one workgroup per row tile walking all of them, and as the model; duplicates of the
    winners at higher indices never win"""
    torch = gpu
    rng = np.random.default_rng(65536)
    cen = rng.standard_normal((65536, 8)).astype(f32)
    rows = (rng.standard_normal((64, 8)) * 0.5).astype(f32)
    rows[:8] = cen[rng.integers(0, 65536, 8)]                                       # distance 0
    first = VM.assign_model(rows, cen)[0]
    low = np.flatnonzero(first[:63] < 60000)
    cen[60000 + low] = cen[first[low]]                                              # a duplicate of those winners, in a later chunk
    cen[100], rows[63, 2] = nan, inf
    want = VM.assign_model(rows, cen)
    assert len(low) > 40 and np.array_equal(want[0][low], first[low]) and want[0][63] == -1
    for wide in BUILDS:
        for splits in (0, 1, 7, 256, 4096):
            assign_case(torch, 8, 65536, 64, wide, splits, 0, rng, cen=cen, rows=rows)


# ------------------------------------------------------------------------------------------------------------------ insert
def archive_bufs(torch, g, offset, rng, G):
    slots = g.M * g.C
    out = dict(elite_fitness=Buf(torch, g.fitness), elite_desc=Buf(torch, g.desc, offset), count=Buf(torch, g.count),
               winner=Buf(torch, np.full((g.M, g.C), 77, np.int32)), scratch=scratch(torch, (12 * slots + 7) // 8 + G, rng))
    for k, name in enumerate(NAMES):
        out["elite_" + name] = Buf(torch, g.weights[k], offset)
    return out


@pytest.mark.parametrize("M", (1, 3))
def test_insert(gpu, M):
    """rem2d_cvt_insert twice, the second on top of the first == cvt_model.insert_model: every grid word, cell, dist, winner and
    count on bits, in the three builds; grids that are empty, partly filled and full (incumbents below, at and above the
    challengers, a NaN among them); masks; forged rows; aligned and offset bases; a forced split"""
    torch = gpu
    seen = dict(held=0, replaced=0, second=0, dropped=0)
    for si, S in enumerate((1, 16, 67)):
        for ci, C_ in enumerate((2, 65)):
            for ki, kind in enumerate(TEL.GRIDS):
                B = WIDTHS[(si + ci + ki + M) % 4]
                shapes = (MIXED, WORK)[(si + ki) % 2] if C_ == 2 else MIXED
                rng = np.random.default_rng([M, S, C_, ki])
                G = M * S
                _, cen = VM.forge(B, C_, 8)
                if C_ == 2:
                    cen[1] = cen[0] + 3                                        # (two cells, not a centroid and its duplicate)
                grid0 = TEL.make_grid(kind, M, C_, B, shapes, rng)
                pops, wants, g = [], [], grid0
                for rnd in range(2):
                    rows = VM.forge(B, C_, G, seed=rnd + 1)[0]
                    rows[G // 2:] = cen[rng.integers(0, C_, G - G // 2)] + (rng.standard_normal((G - G // 2, B)) * 0.25).astype(f32)
                    fitness = TEL.make_rows("random", *TEL.make_map(B, [1], rng), M, S, B, rng)[1]
                    weights = [rng.standard_normal((G,) + s).astype(f32) for s in shapes]
                    weights[0][rng.random(weights[0].shape) < 0.01] = f32(nan)
                    mask = (rng.random(G) < 0.7).astype(np.uint8) if (ki + rnd) % 2 else None
                    g, cell, winner, dist = VM.insert_model(cen, g, weights, fitness, rows, S, mask)
                    pops.append((rows, fitness, weights, mask))
                    wants.append((g, cell, winner, dist))
                cell1, win1 = wants[0][1], wants[0][2]
                cand = np.zeros((M, C_), bool)
                cand[(np.arange(G) // S)[cell1 >= 0], cell1[cell1 >= 0]] = True
                seen["held"] += int((cand & (win1 < 0)).sum()); seen["replaced"] += int((win1 >= 0).sum())
                seen["second"] += int((wants[1][2] >= 0).sum()); seen["dropped"] += int((cell1 < 0).sum())
                for bi, wide in enumerate(BUILDS):
                    off_grid, off_pop = (bi + si) % 2, (bi + ci + ki) % 2
                    gb = archive_bufs(torch, grid0, off_grid, rng, G)
                    cb = Buf(torch, cen, off_pop)
                    for rnd, ((rows, fitness, weights, mask), (want, cell, winner, dist)) in enumerate(zip(pops, wants)):
                        pb = dict(desc=Buf(torch, rows, off_pop), fitness=Buf(torch, fitness), cell=Buf(torch, np.full(G, 99, np.int32)),
                                  dist=Buf(torch, np.full(G, 5.0, f32), off_pop), centroids=cb)
                        for k, name in enumerate(NAMES):
                            pb[name] = Buf(torch, weights[k], off_pop)
                        if mask is not None:
                            pb["mask"] = Buf(torch, mask)
                        v = descriptor(dict(gb, **pb), shapes, width=B, n_cells=C_, n_blocks=M, group_size=S, splits=(0, 3)[(rnd + bi) % 2])
                        call(torch, wide, "rem2d_cvt_insert", v)
                        w = "M %d S %d C %d B %d %s grid, build %s, insert %d" % (M, S, C_, B, kind, wide, rnd + 1)
                        assert np.array_equal(pb["cell"].read(), cell), w + ": cell"
                        assert np.array_equal(bits(pb["dist"].read()), bits(dist)), w + ": dist"
                        assert np.array_equal(gb["winner"].read(), winner), w + ": winner"
                        TEL.same_grid(gb, want, w)
                        assert all(pb[k].unchanged() for k in pb if k not in ("cell", "dist")), w + ": an input was written"
                    gb["scratch"].read()
    assert all(v >= 1 for v in seen.values()), seen


# --------------------------------------------------------------------------------------------------------------- emit_line
def line_grid(M_kinds, C_, shapes, rng):
    """one block per kind: 0, 1, 2 or all cells filled"""
    g = TEL.make_grid("empty", len(M_kinds), C_, 2, shapes, rng)
    for b, kind in enumerate(M_kinds):
        if kind == 1:
            g.count[b, C_ // 2] = 2
        elif kind == 2:
            g.count[b, [0, C_ - 1]] = 1
        elif kind == "all":
            g.count[b] = rng.integers(1, 4, C_)
    g.weights[0][rng.random(g.weights[0].shape) < 0.01] = f32(nan)
    g.weights[2][-1, 0, 0], g.weights[3][-1, 0] = f32(-0.0), f32(inf)
    return g


def line_case(torch, g, shapes, n, sigma_iso, sigma_line, seed, gen, off_grid, off_kid, rng, builds=BUILDS):
    M, C_ = g.M, g.C
    sentinel = [rng.standard_normal((n,) + s).astype(f32) for s in shapes]
    kids, parent, parent2, n_filled = VM.line_model(g, n, sigma_iso, sigma_line, seed, gen, before=sentinel)
    per = n // M
    for b in range(M):
        if n_filled[b] == 0:                                                    # a child of an empty block keeps its sentinel
            assert all(np.array_equal(bits(kids[k][b * per:(b + 1) * per]), bits(sentinel[k][b * per:(b + 1) * per])) for k in range(4))
    for wide in builds:
        gb = archive_bufs(torch, g, off_grid, rng, 0)
        eb = dict(parent=Buf(torch, np.full(n, 55, np.int32)), parent2=Buf(torch, np.full(n, 55, np.int32)), n_filled=Buf(torch, np.full(M, 55, np.int32)))
        for k, name in enumerate(NAMES):
            eb["child_" + name] = Buf(torch, sentinel[k], off_kid)
        bufs = {k: v for k, v in dict(gb, **eb).items() if k not in ("winner", "elite_fitness", "elite_desc")}
        v = descriptor(bufs, shapes, width=2, n_cells=C_, n_blocks=M, n_children=n, generation=gen, seed=seed, sigma_iso=sigma_iso, sigma_line=sigma_line)
        call(torch, wide, "rem2d_cvt_emit_line", v)
        what = "C %d n %d sigma_line %r offsets %d/%d build %s" % (C_, n, sigma_line, off_grid, off_kid, wide)
        assert np.array_equal(eb["n_filled"].read(), n_filled), what + ": n_filled"
        assert np.array_equal(eb["parent"].read(), parent), what + ": parent"
        assert np.array_equal(eb["parent2"].read(), parent2), what + ": parent2"
        for k, name in enumerate(NAMES):
            assert np.array_equal(VM.kid_bits(eb["child_" + name].read()), VM.kid_bits(kids[k])), what + ": child_" + name
        TEL.same_grid(gb, g, what + ": the grid after emit_line")
    return kids, parent, parent2


@pytest.mark.parametrize("shape", ["mixed", "work"])
def test_emit_line(gpu, shape):
    """children, parent, parent2 and n_filled == cvt_model.line_model: blocks with 0, 1, 2 and all cells filled, one and five
    children per block, sigma_line positive, negative and +-0, aligned and offset bases (the 16-byte and the one-word walk); the
    workload's set shape with 64 children"""
    torch = gpu
    if shape == "work":
        rng = np.random.default_rng(64)
        g = line_grid((2, "all"), 5, WORK, rng)
        for off in (0, 1):
            line_case(torch, g, WORK, 64, 0.01, 0.2, (7 << 33) + 3, 9, off, off, rng)
        return
    for ci, (C_, per, sigma_line, off_grid, off_kid) in enumerate(((65, 1, 0.2, 0, 0), (65, 5, 0.2, 1, 0), (9, 5, -0.5, 0, 1), (9, 1, 0.0, 1, 1), (9, 5, -0.0, 0, 0))):
        rng = np.random.default_rng([C_, per, ci])
        g = line_grid((0, 1, 2, "all"), C_, MIXED, rng)
        kids, parent, parent2 = line_case(torch, g, MIXED, 4 * per, 0.05, sigma_line, (5 << 40) + ci, 3 + ci, off_grid, off_kid, rng)
        assert (parent[:per] == -1).all() and (parent2[:per] == -1).all() and (parent[per:] >= 0).all()


def test_emit_line_without_a_line_is_emit(gpu):
    """EliteGrid.emit_line(sigma_line=0) writes what EliteGrid.emit(rate=1.0, sigma=sigma_iso) writes, on a grid and on a centroid
    archive, in the three builds; .parents2 is a draw of its own; out= is written in place"""
    torch = gpu
    from gym_rem2d_amd import elites, policy
    like = policy.MLPPolicy.random(4, 16, 32).to("cuda")
    rng = np.random.default_rng(12)
    cen = rng.standard_normal((7, 4)).astype(f32)
    for g in (elites.EliteGrid(2, [(0, -1.0, 1.0, 7)], 4, like=like, device="cuda"), elites.CentroidArchive(2, cen, like=like, device="cuda")):
        pop = policy.MLPPolicy.random(2 * 40, 16, 32, seed=3).to("cuda")
        desc = torch.from_numpy(rng.standard_normal((80, 4)).astype(f32)).to("cuda")
        g.insert(pop, torch.from_numpy(rng.standard_normal(80)).to("cuda"), desc)
        assert int(g.n_filled.min()) >= 2
        for wide in BUILDS:
            a = g.emit(5, seed=9, rate=1.0, sigma=0.03, n_children=10, wide=wide)
            b = g.emit_line(5, seed=9, sigma_iso=0.03, sigma_line=0.0, n_children=10, wide=wide)
            c = g.emit_line(5, seed=9, sigma_iso=0.03, sigma_line=0.2, n_children=10, out=b, wide=wide)
            assert c is b
            a2 = g.emit(5, seed=9, rate=1.0, sigma=0.03, n_children=10, wide=wide)
            b2 = g.emit_line(5, seed=9, sigma_iso=0.03, sigma_line=-0.0, n_children=10, wide=wide)
            assert np.array_equal(a2.parents.cpu().numpy(), b2.parents.cpu().numpy())
            for x, y in zip((a2.w1, a2.b1, a2.w2, a2.b2), (b2.w1, b2.b1, b2.w2, b2.b2)):
                assert np.array_equal(bits(x.cpu().numpy()), bits(y.cpu().numpy()))
            assert not np.array_equal(bits(a.w1.cpu().numpy()), bits(c.w1.cpu().numpy()))          # (the line term moved the children)
            assert (b2.parents2.cpu().numpy() != b2.parents.cpu().numpy()).any() and (b2.parents2.cpu().numpy() >= 0).all()


# ------------------------------------------------------------------------------------------------- the archive, the centroids
def test_centroid_archive(gpu):
    """elites.CentroidArchive: assign / insert / emit_line give the model's bits; the second round allocates nothing; the readings;
    a checkpoint carries the centroids"""
    torch = gpu
    from gym_rem2d_amd import elites, policy
    M, S, B, C_ = 2, 64, 8, 12
    rng = np.random.default_rng(41)
    cen = (rng.standard_normal((C_, B)) * 1.5).astype(f32)
    like = policy.MLPPolicy.random(M * S, 16, 32).to("cuda")
    arch = elites.CentroidArchive(M, cen, like=like, device="cuda")
    model = QM.Grid(M, C_, B, WORK)
    kids = policy.MLPPolicy.random(M * S, 16, 32, seed=1).to("cuda")
    pop, mem = like, []
    for gen in range(1, 4):
        desc = (rng.standard_normal((M * S, B)) * 1.5).astype(f32)
        fit = rng.integers(0, 4, M * S).astype(f64)
        if gen == 1:
            desc[S:] = nan                                                      # block 1 stays empty for a generation
        weights = [t.cpu().numpy() for t in (pop.w1, pop.b1, pop.w2, pop.b2)]
        d = torch.from_numpy(desc).to("cuda")
        winner = arch.insert(pop, torch.from_numpy(fit).to("cuda"), d)
        model, cell, want_winner, dist = VM.insert_model(cen, model, weights, fit, desc, S)
        assert winner is arch.winner and np.array_equal(winner.cpu().numpy(), want_winner) and np.array_equal(arch.cell.cpu().numpy(), cell)
        assert np.array_equal(bits(arch.dist.cpu().numpy()), bits(dist))
        assert np.array_equal(bits(arch.fitness.cpu().numpy()), bits(model.fitness)) and np.array_equal(arch.count.cpu().numpy(), model.count)
        assert np.array_equal(bits(arch.desc.cpu().numpy()), bits(model.desc))
        for k, t in enumerate((arch.w1, arch.b1, arch.w2, arch.b2)):
            assert np.array_equal(bits(t.cpu().numpy()), bits(model.weights[k])), "generation %d, %s" % (gen, NAMES[k])
        out = torch.empty(M * S, dtype=torch.int32, device="cuda")
        dd = torch.empty(M * S, dtype=torch.float32, device="cuda")
        assert arch.assign(d, out=out, dist=dd) is out
        near = VM.assign_model(desc, cen)
        assert np.array_equal(out.cpu().numpy(), near[0]) and np.array_equal(bits(dd.cpu().numpy()), bits(near[1]))
        filled = model.count != 0
        assert arch.n_filled.cpu().tolist() == filled.sum(axis=1).tolist() and (gen > 1 or arch.n_filled.cpu().tolist()[1] == 0)
        assert np.array_equal(arch.coverage().cpu().numpy(), filled.sum(axis=1) / float(C_))
        before = [t.cpu().numpy() for t in (kids.w1, kids.b1, kids.w2, kids.b2)]
        got = arch.emit_line(gen, seed=9, sigma_iso=0.02, sigma_line=0.3, out=kids, wide=BUILDS[gen - 1])
        assert got is kids
        want, parent, parent2, n_filled = VM.line_model(model, M * S, 0.02, 0.3, 9, gen, before=before)
        assert np.array_equal(kids.parents.cpu().numpy(), parent) and np.array_equal(kids.parents2.cpu().numpy(), parent2)
        assert np.array_equal(arch.filled.cpu().numpy(), n_filled)
        for k, t in enumerate((kids.w1, kids.b1, kids.w2, kids.b2)):
            assert np.array_equal(VM.kid_bits(t.cpu().numpy()), VM.kid_bits(want[k])), "generation %d, child %s" % (gen, NAMES[k])
        assert np.array_equal(arch.sample(gen, seed=9, n_children=M * S).cpu().numpy(), parent)     # the older draw sees a grid of C bins
        pop = kids
        del out, dd, d
        torch.cuda.synchronize()
        mem.append(torch.cuda.memory_allocated())
    assert mem[2] == mem[1], mem
    state = arch.state_dict()
    other = elites.CentroidArchive(M, np.zeros_like(cen), like=like, device="cuda")
    other.load_state_dict(state)
    assert np.array_equal(other.centroids.cpu().numpy(), cen) and np.array_equal(other.count.cpu().numpy(), model.count)
    a, b = arch.emit_line(7, n_children=M * 3), other.emit_line(7, n_children=M * 3)
    assert np.array_equal(bits(a.w1.cpu().numpy()), bits(b.w1.cpu().numpy())) and np.array_equal(a.parents2.cpu().numpy(), b.parents2.cpu().numpy())


def test_cvt_centroids_on_the_gpu_are_the_cpus(gpu):
    """64 centroids of 8 words from 2 048 points in 5 rounds: the assignment is bit-defined, so both routes return the same bits"""
    torch = gpu
    from gym_rem2d_amd import elites
    lo, hi = [3.0, 5.0] * 4, [7.0, 6.0] * 4
    cpu = elites.cvt_centroids(64, lo, hi, n_samples=2048, iterations=5, seed=2)
    for wide in BUILDS:
        dev = elites.cvt_centroids(64, lo, hi, n_samples=2048, iterations=5, seed=2, device="cuda", wide=wide)
        assert dev.device.type == "cuda" and np.array_equal(bits(dev.cpu().numpy()), bits(cpu.numpy())), wide
    assert not np.array_equal(cpu.numpy(), elites.cvt_centroids(64, lo, hi, n_samples=2048, iterations=4, seed=2).numpy())


# ------------------------------------------------------------------------------------------------------------------ the loop
def test_two_generations_over_a_centroid_archive(gpu):
    """evaluate.run_policy_map_elites with a CentroidArchive and sigma_line on 2 morphology blocks x 8 creatures, episodes of 32
    steps described 4 times: an on_generation hook keeps the device's own fitness, behaviour and children, and after every
    generation the archive, the cells and the children are cvt_model's insert / line fed those -- the plumbing of seed, generation
    and order"""
    torch = gpu
    from gym_rem2d_amd import elites, evaluate, make_terrain, policy, synthetic  # noqa: F401
    from gym_rem2d_amd.compiler import Morphology, lanes_for
    from gym_rem2d_amd.env import BatchedModular2D
    specs = [s for s in synthetic.lsystem_specs(range(60)) if s.n_bodies >= 2][:16]
    n, S, K, steps, period, seed, sigma, sigma_line = 16, 8, 4, 32, 8, 7, 0.05, 0.3
    groups = {}
    for e, s in enumerate(specs):
        groups.setdefault(lanes_for(s.n_bodies), []).append(e)
    batches = [(Morphology.from_specs([specs[e] for e in groups[g]], g), groups[g]) for g in sorted(groups)]
    W = list(PM.loop_weights(n, 16))
    cen = elites.cvt_centroids(6, [3.0, 5.0] * K, [7.0, 6.0] * K, n_samples=256, iterations=3, seed=1).numpy()
    env = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
    try:
        env.reset_batches(batches, n)
        first = policy.MLPPolicy(*[torch.from_numpy(a.copy()) for a in W]).to("cuda")
        arch = elites.CentroidArchive(n // S, cen, like=first, device="cuda")
        seen = []

        def keep(g, kids, f, b, gr):
            seen.append(dict(kids=[t.cpu().numpy() for t in (kids.w1, kids.b1, kids.w2, kids.b2)], fit=f.cpu().numpy(), beh=b.cpu().numpy(),
                             parent=None if g == 0 else kids.parents.cpu().numpy(), parent2=None if g == 0 else kids.parents2.cpu().numpy(),
                             cell=gr.cell.cpu().numpy(), winner=gr.winner.cpu().numpy(), state={k: v.cpu().numpy() for k, v in gr.state_dict().items()}))
        got, fit, history = evaluate.run_policy_map_elites(env, first, arch, 2, period=period, samples=K, seed=seed, sigma=sigma, group_size=S,
                                                           max_steps=steps, on_generation=keep, sigma_line=sigma_line)
        assert got is arch and len(seen) == 3 and [h[0] for h in history] == [0, 1, 2]
        model = QM.Grid(n // S, 6, 2 * K, [a.shape[1:] for a in W])
        for g, s in enumerate(seen):
            if g == 0:
                assert all(np.array_equal(bits(s["kids"][k]), bits(W[k])) for k in range(4))
            else:
                want, parent, parent2, _ = VM.line_model(model, n, sigma, sigma_line, seed, g, before=seen[g - 1]["kids"])
                assert np.array_equal(s["parent"], parent) and np.array_equal(s["parent2"], parent2), "generation %d: parents" % g
                for k in range(4):
                    assert np.array_equal(VM.kid_bits(s["kids"][k]), VM.kid_bits(want[k])), "generation %d: children, %s" % (g, NAMES[k])
            model, cell, winner, _ = VM.insert_model(cen, model, s["kids"], s["fit"], s["beh"], S)
            assert np.array_equal(s["cell"], cell) and np.array_equal(s["winner"], winner), "generation %d: cell, winner" % g
            for key, arr in (("fitness", model.fitness), ("desc", model.desc), ("count", model.count), ("w1", model.weights[0]), ("b1", model.weights[1]),
                             ("w2", model.weights[2]), ("b2", model.weights[3]), ("centroids", cen)):
                assert np.array_equal(bits(s["state"][key]), bits(arr)), "generation %d: the archive's %s" % (g, key)
            assert history[g][4] == int((model.count != 0).sum())
        assert (model.count != 0).sum(axis=1).min() >= 1 and (seen[1]["parent"] >= 0).all()
        assert np.array_equal(bits(fit.cpu().numpy()), bits(seen[2]["fit"])) and np.array_equal(bits(first.w1.cpu().numpy()), bits(W[0]))
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------ the caller's stream
ST_B, ST_C, ST_M, ST_S, ST_S2, ST_ROWS = 3, 5, 2, 5, 6, 70
ST_ISO, ST_LINE, ST_GEN, ST_SEED = 0.25, 0.5, 13, (7 << 33) + 1


def stream_case(torch, wide, which):
    """one of the three calls through the Python layer, as test_caller_stream_gpu's cases are built: three data sets (A, B and a
    finite decoy), outputs under sentinels, the numpy model as the reference"""
    from gym_rem2d_amd import elites, policy
    shapes = MIXED
    M, S, G, C_, B = ST_M, ST_S, ST_M * ST_S, ST_C, ST_B
    c = TCS.Case(torch)
    rays = np.zeros((3, 2)) + 1.0
    like = policy.MLPPolicy(*[torch.zeros((1,) + sh, dtype=torch.float32, device=c.dev) for sh in shapes], rays=rays)
    sets = []
    for s in (1, 2, 3):
        rng = np.random.default_rng([s, 77])
        cen = rng.standard_normal((C_, B)).astype(f32)
        n = ST_ROWS if which == "assign" else G
        rows = (cen[rng.integers(0, C_, n)] + rng.standard_normal((n, B)) * 0.3).astype(f32)
        g = TEL.make_grid(("partly", "partly", "full")[s - 1], M, C_, B, shapes, rng)
        g.count[:, 0] = 1                                                       # (no block is empty: a decoy changes every child)
        fitness = TEL.make_rows("random", *TEL.make_map(B, [1], rng), M, S, B, rng)[1]
        weights = [rng.standard_normal((G,) + sh).astype(f32) for sh in shapes]
        if s == 3:
            g.fitness, fitness = TCS._finite(g.fitness, rng), TCS._finite(fitness, rng)
        else:
            rows[1, 0] = nan
        sets.append(dict(cen=cen, rows=rows, grid=g, fitness=fitness, weights=weights))
    arch = elites.CentroidArchive(M, sets[0]["cen"], like=like, device=c.dev)
    n_kids = M * ST_S2
    if which != "line":
        c.bind("centroids", arch.centroids, *(s["cen"] for s in sets))
        desc = c.inp("desc", *(s["rows"] for s in sets))
    if which == "assign":
        cell = c.out("cell", (ST_ROWS,), torch.int32, TCS.I_SENT)
        dist = c.out("dist", (ST_ROWS,), torch.float32, TCS.F_SENT)
        arch._vscratch = torch.empty(ST_ROWS, dtype=torch.int64, device=c.dev)
        c.call = lambda: arch.assign(desc, out=cell, dist=dist, wide=wide, splits=2)

        def want_assign(key):
            near, d = VM.assign_model(c.data[key]["desc"], c.data[key]["centroids"])
            return [near, bits(d)]
        c.want = want_assign
        c.norm = lambda key, got: [got[0], bits(got[1])]
        return c
    c.bind("count", arch.count, *(s["grid"].count for s in sets))
    for k, name in enumerate(TCS.NAMES4):
        c.bind("elite_" + name, getattr(arch, name), *(s["grid"].weights[k] for s in sets))

    def grid_of(key):
        d = c.data[key]
        g = QM.Grid(M, C_, B, shapes)
        g.count[:] = d["count"]
        for k, name in enumerate(TCS.NAMES4):
            g.weights[k].view(np.uint32)[:] = d["elite_" + name].view(np.uint32)
        return g, d
    if which == "insert":
        c.bind("elite_fitness", arch.fitness, *(s["grid"].fitness for s in sets))
        c.bind("elite_desc", arch.desc, *(s["grid"].desc for s in sets))
        fit = c.inp("fitness", *(s["fitness"] for s in sets))
        pop = policy.MLPPolicy(*[c.inp(name, *(s["weights"][k] for s in sets)) for k, name in enumerate(TCS.NAMES4)], rays=rays)
        arch.cell = c.out("cell", (G,), torch.int32, TCS.I_SENT)
        arch.dist = c.out("dist", (G,), torch.float32, TCS.F_SENT)
        c.out_existing("winner", arch.winner, TCS.I_SENT)
        for name in ("elite_fitness", "elite_desc", "count") + tuple("elite_" + x for x in TCS.NAMES4):
            c.inout(name)
        arch._vscratch = torch.empty((12 * M * C_ + 8 * G + 7) // 8, dtype=torch.int64, device=c.dev)
        c.call = lambda: arch.insert(pop, fit, desc, group_size=S, wide=wide)

        def want(key):
            g, d = grid_of(key)
            g.fitness[:], g.desc[:] = d["elite_fitness"], d["elite_desc"]
            out, cell, winner, dist = VM.insert_model(d["centroids"], g, [d[x] for x in TCS.NAMES4], d["fitness"], d["desc"], S)
            return [cell, bits(dist), winner, bits(out.fitness), bits(out.desc), np.asarray(out.count, np.int32)] + [bits(w) for w in out.weights]
        c.want = want
        c.norm = lambda key, got: [got[0], bits(got[1]), got[2], bits(got[3]), bits(got[4]), got[5]] + [bits(w) for w in got[6:]]
        return c
    parent = c.out("parent", (n_kids,), torch.int32, TCS.I_SENT)
    parent2 = c.out("parent2", (n_kids,), torch.int32, TCS.I_SENT)
    c.out_existing("n_filled", arch.filled, TCS.I_SENT)
    child = policy.MLPPolicy(*[c.out("child_" + name, (n_kids,) + shapes[k], torch.float32, TCS.F_SENT) for k, name in enumerate(TCS.NAMES4)], rays=rays)
    child.parents, child.parents2 = parent, parent2
    c.call = lambda: arch.emit_line(ST_GEN, ST_SEED, ST_ISO, ST_LINE, n_kids, out=child, wide=wide)

    def want_line(key):
        g, _ = grid_of(key)
        kids, p, p2, n_filled = VM.line_model(g, n_kids, ST_ISO, ST_LINE, ST_SEED, ST_GEN, before=[np.full((n_kids,) + sh, TCS.F_SENT, f32) for sh in shapes])
        return [p, p2, n_filled] + [VM.kid_bits(k) for k in kids]
    c.want = want_line
    c.norm = lambda key, got: got[:3] + [VM.kid_bits(k) for k in got[3:]]
    return c


_CASES = {}


def _stream_case(torch, which, build):
    if (which, build) not in _CASES:
        c = stream_case(torch, build, which)
        memo, model = {}, c.want
        c.want = lambda key: memo[key] if key in memo else memo.setdefault(key, model(key))
        _CASES[(which, build)] = c
    return _CASES[(which, build)]


@pytest.fixture(scope="module", autouse=True)
def _cases_released():
    yield
    _CASES.clear()


STREAM_IDS = [pytest.param(w, b, id="%s-%s" % (w, TCS._bid(b))) for w in ("assign", "insert", "line") for b in BUILDS]


@pytest.mark.parametrize("which,build", STREAM_IDS)
def test_capture_and_replay(gpu, which, build):
    """The call alone captured on a caller's stream (the stream travels in the descriptor): the capture succeeds -- nothing
    synchronised, allocated through HIP or touched the legacy stream --, nothing ran during it, and each replay computes the model's
    result of what the inputs hold then: data set A, then B written in place"""
    torch = gpu
    c = _stream_case(torch, which, build)
    what = "rem2d_cvt_%s (%s build)" % (which, TCS._bid(build))
    c.load("A")
    torch.cuda.synchronize()
    before = c.read()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.call()
    torch.cuda.synchronize()
    c.untouched("A", before, what + " during capture")
    g.replay()
    torch.cuda.synchronize()
    c.compare("A", what + " first replay")
    c.load("B")
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    c.compare("B", what + " second replay")
    del g


@pytest.mark.parametrize("which,build", STREAM_IDS)
def test_behind_a_gate(gpu, gate, which, build):  # noqa: F811
    """test_caller_stream_gpu's gate leg, as it is: the call on a caller's stream behind a spin and the copies that bring its real
    inputs; a launch that went to any other stream reads the decoy"""
    torch = gpu
    c = _stream_case(torch, which, build)
    c.reads_decoy()
    TCS._gated(torch, c, gate)
    what = "rem2d_cvt_%s (%s build) behind the gate" % (which, TCS._bid(build))
    got, decoy = c.norm("decoy", c.read()), c.want("decoy")
    for n, g, d in zip(c.names(), got, decoy):
        assert n in c.insensitive or (np.asarray(g).reshape(-1) != np.asarray(d).reshape(-1)).any(), \
            "%s: `%s` holds the DECOY's result: a launch did not wait for the caller's stream" % (what, n)
    c.compare("A", what)


# ------------------------------------------------------------------------------------------------------------- error paths
def test_refusals_write_nothing(gpu):
    """REM2D_E_INVALID for the refusals the header lists, on real device buffers: overlapping child and elite buffers among them;
    nothing is written after a refusal -- outputs, grid and scratch hold what they held"""
    torch = gpu
    rng = np.random.default_rng(3)
    M, S, C_, B, G = 2, 4, 5, 3, 8
    rows, cen = VM.forge(B, C_, G)
    g = TEL.make_grid("partly", M, C_, B, MIXED, rng)
    for wide in BUILDS:
        gb = archive_bufs(torch, g, 0, rng, G)
        pb = dict(desc=Buf(torch, rows), centroids=Buf(torch, cen), fitness=Buf(torch, rng.standard_normal(G)), cell=Buf(torch, np.full(G, 99, np.int32)),
                  dist=Buf(torch, np.full(G, 5.0, f32)), parent=Buf(torch, np.full(G, 55, np.int32)), parent2=Buf(torch, np.full(G, 55, np.int32)),
                  n_filled=Buf(torch, np.full(M, 55, np.int32)))
        for k, name in enumerate(NAMES):
            pb[name] = Buf(torch, rng.standard_normal((G,) + MIXED[k]).astype(f32))
            pb["child_" + name] = Buf(torch, rng.standard_normal((G,) + MIXED[k]).astype(f32))
        bufs = dict(gb, **pb)
        good = dict(width=B, n_cells=C_, n_blocks=M, group_size=S, n_children=G, n_rows=G, sigma_iso=0.1, sigma_line=0.2)

        class At:                                                               # (a stand-in Buf at another buffer's address)
            def __init__(self, ptr):
                self.ptr = ptr
        cases = [("rem2d_cvt_assign", dict(width=0), {}, b"width"), ("rem2d_cvt_assign", dict(n_cells=65537), {}, b"n_cells"),
                 ("rem2d_cvt_assign", dict(n_rows=0), {}, b"n_rows"), ("rem2d_cvt_assign", dict(splits=4097), {}, b"splits"),
                 ("rem2d_cvt_assign", dict(scratch_bytes=8 * G - 1), {}, b"scratch holds"), ("rem2d_cvt_assign", dict(reserved=1), {}, b"reserved"),
                 ("rem2d_cvt_assign", {}, dict(desc=At(bufs["cell"].ptr)), b"desc overlaps cell"), ("rem2d_cvt_assign", {}, dict(cell=At(0)), b"NULL device pointer (cell)"),
                 ("rem2d_cvt_insert", dict(group_size=0), {}, b"group_size"), ("rem2d_cvt_insert", dict(hidden=0), {}, b"hidden"),
                 ("rem2d_cvt_insert", dict(scratch_bytes=12 * M * C_ + 8 * G - 1), {}, b"scratch holds"),
                 ("rem2d_cvt_insert", {}, dict(desc=At(bufs["elite_desc"].ptr)), b"desc overlaps elite_desc"),
                 ("rem2d_cvt_insert", {}, dict(w1=At(bufs["elite_w1"].ptr)), b"elite_w1 overlaps the evaluated sets' w1"),
                 ("rem2d_cvt_insert", {}, dict(fitness=At(0)), b"NULL device pointer (fitness)"),
                 ("rem2d_cvt_emit_line", dict(n_children=3), {}, b"n_children"), ("rem2d_cvt_emit_line", dict(sigma_line=inf), {}, b"sigma_line"),
                 ("rem2d_cvt_emit_line", {}, dict(child_w1=At(bufs["elite_w1"].ptr)), b"child_w1 overlaps elite_w1"),
                 ("rem2d_cvt_emit_line", {}, dict(child_b2=At(bufs["elite_w2"].ptr + 16)), b"child_b2 overlaps elite_w2"),
                 ("rem2d_cvt_emit_line", {}, dict(parent2=At(0)), b"NULL device pointer (parent2)"),
                 ("rem2d_cvt_emit_line", {}, dict(scratch=At(bufs["scratch"].ptr + 4)), b"8-byte aligned")]
        for name, fields, swaps, msg in cases:
            use = dict(bufs)
            use.update(swaps)
            v = descriptor(use, MIXED, **dict(good, **fields))
            if "scratch_bytes" not in fields:
                v.scratch_bytes = bufs["scratch"].n * 8
            err = call(torch, wide, name, v, expect=-1)
            assert msg in err, (name, fields, err)
        assert all(b.unchanged() for b in bufs.values()), "a refused call wrote something (build %s)" % (wide,)
        # and the same descriptor, good, is taken
        call(torch, wide, "rem2d_cvt_assign", descriptor(bufs, MIXED, **good))
        assert np.array_equal(bufs["cell"].read(), VM.assign_model(rows, cen)[0])
