"""MAP-Elites for device policies without a GPU (include/rem2d_elites.h): a host model with teeth, the header's worked examples, the
header, the ctypes binding and the three libraries in agreement, the argument checks of the entry points and the value errors of the
Python layer, and MAP-Elites doing what it is for on DESIGN.md 17's deceptive toy.

The GPU half (tests/test_elites_gpu.py) compares the kernels with tests/elites_model.py bit for bit; this half makes sure that the
model is no vacuous yardstick."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import elites_model as QM
import es_model as ES
import evolve_model as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
nan, inf = np.nan, np.inf
SMALL = ((17 - 3, 1), (1,), (1, 1), (1,))                  # the smallest policy shape: MB 1, R 0, H 1 -- 17 words per set


# ------------------------------------------------------------------------------------------------------------------- teeth
def teeth_inputs():
    """3 blocks of 96 rows over a 4 x 3 grid on words 1 and 0 of 2 (asymmetric, so reversed strides show): fitness on a coarse
    integer grid with both zeros (ties within a cell, ties with the incumbents), descriptors on cell edges, on half-way points and
    outside [lo, hi) -- block 1's fitness is -1 and the two zeros alone, so that the zeros meet; a grid whose every cell of block 0
    is filled with fitness 1 (= a frequent challenger), of block 1 with -0 and -1 in turn, and whose block 2 is a quarter filled"""
    rng = np.random.default_rng(11)
    M, S, B = 3, 96, 2
    cmap = QM.CellMap.of([(1, -1.0, 1.0, 4), (0, 0.0, 3.0, 3)])
    desc = (rng.integers(-6, 11, (M * S, B)) * 0.25).astype(f32)       # multiples of 1/4 in [-1.5, 2.5]: edges, halves, outside
    fitness = rng.integers(-1, 3, M * S).astype(np.float64)
    fitness[rng.random(M * S) < 0.15] = -0.0
    fitness[S:2 * S] = rng.choice([-1.0, 0.0, -0.0], S)
    weights = [rng.standard_normal((M * S,) + s).astype(f32) for s in SMALL]
    grid = QM.Grid(M, cmap.n_cells, B, SMALL)
    grid.count[0], grid.fitness[0] = 1, 1.0
    grid.count[1], grid.fitness[1, 0::2], grid.fitness[1, 1::2] = 2, -0.0, -1.0
    grid.count[2, ::4], grid.fitness[2, ::4] = 1, -5.0
    return cmap, grid, weights, fitness, desc, S


def variant_shares():
    cmap, grid, weights, fitness, desc, S = teeth_inputs()
    right, cell, winner = QM.insert_model(cmap, grid, weights, fitness, desc, S)
    n_filled, parent = QM.sample_model(right.count, 3 * 64, 5, 1)
    shares = {}
    for v in QM.VARIANTS:
        wrong, wcell, wwinner = QM.insert_model(cmap, grid, weights, fitness, desc, S, variant=v)
        _, wparent = QM.sample_model(right.count, 3 * 64, 5, 1, variant=v)
        got = np.concatenate([wrong.words(), wcell.view(np.uint32), wwinner.view(np.uint32).ravel(), wparent.view(np.uint32)])
        want = np.concatenate([right.words(), cell.view(np.uint32), winner.view(np.uint32).ravel(), parent.view(np.uint32)])
        shares[v] = float((got != want).mean())
    return shares


def test_the_model_has_teeth():
    """What a kernel could get wrong shows in the bits of the grid, of cell, winner and parent: ties to the highest row, replacement
    on equal fitness, u rounded instead of truncated, the strides in reverse dimension order, out-of-range rows dropped, the draw
    over all cells, -0 ordered below +0"""
    shares = variant_shares()
    print("share of output words that change: %s" % ", ".join("%s %.2f %%" % (v, 100 * s) for v, s in shares.items()))
    assert set(shares) == set(QM.VARIANTS)
    for v, s in shares.items():
        assert s > 0.0, v


def test_vectorised_emit_is_evolve_models_mutation():
    """elites_model.emit_model mutates all children of an array at once; one child at a time through evolve_model.mutate_set is the
    same bits"""
    rng = np.random.default_rng(3)
    shapes = ((20, 3), (3,), (3, 2), (2,))
    grid = QM.Grid(2, 5, 1, shapes)
    grid.count[0, [1, 4]] = 1
    for w in grid.weights:
        w[:] = rng.standard_normal(w.shape)
    grid.weights[0][1, 0, 0], grid.weights[0][4, 1, 1] = nan, -0.0
    before = [np.full((6,) + s, 7.0, f32) for s in shapes]
    kids, hits, parent, n_filled = QM.emit_model(grid, 6, EM.rate_threshold(0.4), 0.1, 9, 2, before=before)
    assert n_filled.tolist() == [2, 0] and set(parent[:3].tolist()) <= {1, 4} and parent[3:].tolist() == [-1] * 3
    for c in range(6):
        for k in range(4):
            if parent[c] < 0:
                assert (kids[k][c] == 7.0).all() and not hits[k][c].any()
                continue
            want, hit = EM.mutate_set(grid.weights[k][parent[c]], c, EM.W1_DOMAIN + k, EM.rate_threshold(0.4), 0.1, 9, 2)
            assert np.array_equal(EM.bits(kids[k][c], hit), EM.bits(want, hit)) and np.array_equal(hits[k][c], hit)
    assert 0.2 < np.mean([h[:3].mean() for h in hits]) < 0.6


# ---------------------------------------------------------------------------------------------------- the header's examples
def test_the_headers_worked_examples():
    cmap = QM.CellMap([0], [4], [0.0], [1.0])
    grid = QM.Grid(1, 4, 1, SMALL)
    grid.count[0, 3], grid.fitness[0, 3], grid.desc[0, 3, 0] = 1, 9.0, 3.5
    weights = [np.arange(4 * int(np.prod(s)), dtype=f32).reshape((4,) + s) + 1 for s in SMALL]
    desc, fitness = np.array([[0.5], [0.25], [2.0], [7.0]], f32), np.array([1.0, 1.0, -0.0, 5.0])
    after, cell, winner = QM.insert_model(cmap, grid, weights, fitness, desc, 4)
    assert cell.tolist() == [0, 0, 2, 3] and winner.tolist() == [[0, -1, 2, -1]]
    assert after.count.tolist() == [[1, 0, 1, 1]] and after.fitness[0, 3] == 9.0 and after.desc[0, 3, 0] == 3.5
    assert after.fitness[0, 0] == 1.0 and np.signbit(after.fitness[0, 2]) and after.desc[0, :3, 0].tolist() == [0.5, 0.0, 2.0]
    assert all(np.array_equal(after.weights[k][0], weights[k][0]) and np.array_equal(after.weights[k][2], weights[k][2]) for k in range(4))
    assert all((after.weights[k][[1, 3]] == 0).all() for k in range(4))
    again, cell2, winner2 = QM.insert_model(cmap, after, weights, fitness, desc, 4)
    assert np.array_equal(again.words(), after.words()) and (winner2 == -1).all() and cell2.tolist() == cell.tolist()
    # +0 does not replace -0, a strictly better row does, NaN and masked rows and non-finite words are not admitted
    f3 = np.array([0.0, nan, 2.0, 6.0])
    d3 = np.array([[2.5], [1.0], [0.0], [nan]], f32)
    a3, c3, w3 = QM.insert_model(cmap, after, weights, f3, d3, 4, mask=[1, 1, 1, 1])
    assert c3.tolist() == [2, -1, 0, -1] and w3.tolist() == [[2, -1, -1, -1]] and a3.count.tolist() == [[2, 0, 1, 1]]
    assert QM.insert_model(cmap, after, weights, f3, d3, 4, mask=[1, 1, 0, 1])[2].tolist() == [[-1] * 4]
    # +-inf are fitness values; beyond both ends and near 1e19 a row lands in the border cells
    f4 = np.array([-inf, inf, 0.0, 0.0])
    d4 = np.array([[-1e19], [1e19], [-0.0], [4.0]], f32)
    a4, c4, w4 = QM.insert_model(cmap, QM.Grid(1, 4, 1, SMALL), weights, f4, d4, 4)
    assert c4.tolist() == [0, 3, 0, 3] and w4.tolist() == [[2, -1, -1, 1]] and a4.fitness[0].tolist() == [0.0, 0.0, 0.0, inf]
    # an incumbent NaN (a loaded checkpoint) is below everything, -inf included
    g5 = QM.Grid(1, 4, 1, SMALL)
    g5.count[0, 0], g5.fitness[0, 0] = 1, nan
    assert QM.insert_model(cmap, g5, weights, f4, d4, 4)[2].tolist() == [[2, -1, -1, 1]]
    # the strides: dimension 0 is the fastest
    cm2 = QM.CellMap.of([(0, 0.0, 2.0, 2), (1, 0.0, 3.0, 3)])
    assert QM.cells_model(cm2, np.array([[1.5, 0.5], [0.5, 2.5], [1.0, 1.0]], f32), np.zeros(3)).tolist() == [1, 4, 3]
    # the draw: cells 1 and 5 of 8; an empty block
    count = np.zeros((2, 8), np.int32)
    count[0, [1, 5]] = 3
    n_filled, parent = QM.sample_model(count, 2 * 256, 4, 7)
    x0 = EM.philox((0, np.arange(256), 7, 10), EM.seed_key(4))[0]
    assert n_filled.tolist() == [2, 0] and np.array_equal(parent[:256], np.where(x0 < 2 ** 31, 1, 5)) and (parent[256:] == -1).all()
    assert 90 < (parent[:256] == 1).sum() < 166 and QM.ELITES_DOMAIN == 10
    other = [QM.sample_model(count, 512, s, g)[1] for s, g in ((4, 8), (5, 7))]
    assert all((o != parent).any() for o in other)


# -------------------------------------------------------------------------------------------- header, binding, libraries
EXPORTS = ["rem2d_elites_abi_version", "rem2d_elites_scratch_bytes", "rem2d_elites_insert", "rem2d_elites_sample", "rem2d_elites_emit"]


def test_header_binding_and_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    with open(os.path.join(ROOT, "include", "rem2d_elites.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*(?:int|int64_t)\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert declared == EXPORTS
    assert int(re.search(r"#define REM2D_ELITES_ABI_VERSION (\d+)", text).group(1)) == _lib.ELITES_ABI_VERSION == 1
    for name, value in (("MAX_WIDTH", _lib.ELITES_MAX_WIDTH), ("MAX_DIMS", _lib.ELITES_MAX_DIMS), ("MAX_CELLS", _lib.ELITES_MAX_CELLS)):
        assert int(re.search(r"#define REM2D_ELITES_%s (\d+)" % name, text).group(1)) == value
    assert _lib.ELITES_MAX_CELLS == QM.MAX_CELLS == 65536
    for const in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "generation, 10)", "CPU twin has no counterpart"):
        assert const in text, const
    body = re.search(r"typedef struct rem2d_elites \{(.*?)\} rem2d_elites;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)(\[4\])?;", body, flags=re.M)
    assert [m[2] for m in members] == [n for n, _ in _lib.Elites._fields_], members
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
    for (tname, star, name, arr), (_, ct) in zip(members, _lib.Elites._fields_):
        want = C.c_void_p if star else ctype[tname]
        assert (ct._type_ is want and ct._length_ == 4) if arr else (ct is want), name
    assert C.sizeof(_lib.Elites) == 8 * 4 + 4 * 16 + 2 * 4 + 2 * 8 + 23 * 8 + 8 + 8
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in declared:
            assert (" T " + name) in syms, (path, name)
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        assert L.rem2d_elites_abi_version() == _lib.ELITES_ABI_VERSION
        assert L.rem2d_abi_version() == 11 and L.rem2d_evolve_abi_version() == 1 and L.rem2d_novelty_abi_version() == 1
    # the older headers know nothing of it
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header == "rem2d_elites.h":
            continue
        with open(os.path.join(ROOT, "include", header)) as f:
            other = f.read()
        for name in declared + ["REM2D_ELITES_", "rem2d_elites"]:
            assert name not in other, (header, name)


POINTERS = ("desc", "fitness", "mask", "w1", "b1", "w2", "b2", "elite_fitness", "elite_desc", "elite_w1", "elite_b1", "elite_w2",
            "elite_b2", "count", "cell", "winner", "child_w1", "child_b1", "child_w2", "child_b2", "parent", "n_filled", "scratch")
AT = {k: (i + 1) << 26 for i, k in enumerate(POINTERS)}      # the "device pointers", 64 MB apart
G_, M_, S_, C_, B_, D_, H_, MB_ = 64, 4, 16, 16, 8, 114, 32, 16
LEN = dict(w1=D_ * H_, b1=H_, w2=H_ * MB_, b2=MB_)
DESC_BYTES = G_ * B_ * 4
NEED = 12 * M_ * C_


def _desc(**kw):
    """a good descriptor: 4 blocks of 16 rows of 8 words, a 4 x 4 grid, the workload's policy shape, 64 children; the "device
    pointers" are never dereferenced: the checks come first"""
    from gym_rem2d_amd import _lib
    e = _lib.Elites()
    e.d, e.hidden, e.max_bodies, e.width, e.n_blocks, e.group_size, e.n_children, e.n_dims = D_, H_, MB_, B_, M_, S_, G_, 2
    for i, (w, b, lo, inv) in enumerate(((0, 4, -1.0, 2.0), (7, 4, 0.0, 0.5))):
        e.word[i], e.bins[i], e.lo[i], e.inv[i] = w, b, lo, inv
    e.generation, e.sigma, e.rate_threshold, e.seed, e.reserved = 3, 0.1, 2 ** 32, 2 ** 64 - 1, 0
    for k in POINTERS:
        setattr(e, k, AT[k])
    e.scratch_bytes = NEED
    for k, v in kw.items():
        if isinstance(v, dict):
            for i, x in v.items():
                getattr(e, k)[i] = x
        else:
            setattr(e, k, v)
    return e


SHAPE_CASES = [(dict(max_bodies=0), b"max_bodies"), (dict(max_bodies=65), b"max_bodies"), (dict(hidden=0), b"hidden"), (dict(hidden=129), b"hidden"),
               (dict(d=103), b"d must be"), (dict(d=169), b"d must be"), (dict(width=0), b"width"), (dict(width=33), b"width"),
               (dict(n_blocks=0), b"n_blocks"), (dict(n_blocks=-4), b"n_blocks"), (dict(n_dims=0), b"n_dims"), (dict(n_dims=5), b"n_dims"),
               (dict(word={0: -1}), b"word[0]"), (dict(word={1: 8}), b"word[1]"), (dict(bins={0: 0}), b"bins[0]"), (dict(bins={1: -4}), b"bins[1]"),
               (dict(bins={0: 257, 1: 256}), b"product of bins"), (dict(bins={0: 65536, 1: 65536}), b"product of bins"),
               (dict(n_blocks=32768, bins={0: 256, 1: 256}), b"n_blocks times the cells"),
               (dict(lo={0: nan}), b"lo[0]"), (dict(lo={1: inf}), b"lo[1]"), (dict(lo={1: -inf}), b"lo[1]"),
               (dict(inv={0: 0.0}), b"inv[0]"), (dict(inv={0: -1.0}), b"inv[0]"), (dict(inv={1: nan}), b"inv[1]"), (dict(inv={1: inf}), b"inv[1]"),
               (dict(rate_threshold=2 ** 32 + 1), b"rate_threshold"), (dict(rate_threshold=2 ** 64 - 1), b"rate_threshold"),
               (dict(reserved=1), b"reserved"), (dict(reserved=-1), b"reserved")]
SCRATCH_CASES = [(dict(count=None), b"NULL device pointer (count)"), (dict(scratch=None), b"NULL device pointer (scratch)"),
                 (dict(scratch=AT["scratch"] + 4), b"8-byte aligned"), (dict(scratch_bytes=NEED - 1), b"scratch holds"), (dict(scratch_bytes=0), b"scratch holds")]
INSERT_CASES = ([(dict(group_size=0), b"group_size"), (dict(group_size=-16), b"group_size"), (dict(n_blocks=2 ** 16, group_size=2 ** 15, bins={0: 1, 1: 1}), b"n_blocks * group_size")]
                + [(dict(**{k: None}), ("NULL device pointer (%s)" % k).encode()) for k in ("desc", "fitness", "elite_fitness", "elite_desc", "cell", "winner")]
                + [(dict(**{k: None}), b"NULL device pointer (weights)") for k in ("w1", "b1", "w2", "b2", "elite_w1", "elite_b1", "elite_w2", "elite_b2")]
                + [(dict(desc=AT[k]), ("desc overlaps %s" % k).encode()) for k in ("elite_fitness", "elite_desc", "count", "elite_w1", "elite_b1", "elite_w2", "elite_b2")]
                + [(dict(desc=AT["elite_desc"] + M_ * C_ * B_ * 4 - 4), b"desc overlaps elite_desc"), (dict(desc=AT["count"] - DESC_BYTES + 4), b"desc overlaps count"),
                   (dict(w1=AT["elite_w1"]), b"elite_w1 overlaps the evaluated sets' w1"), (dict(b2=AT["elite_w2"] + 64), b"elite_w2 overlaps the evaluated sets' b2"),
                   (dict(w2=AT["elite_b1"] - G_ * LEN["w2"] * 4 + 4), b"elite_b1 overlaps the evaluated sets' w2")])
SAMPLE_CASES = [(dict(n_children=0), b"n_children"), (dict(n_children=-4), b"n_children"), (dict(n_children=66), b"n_children"),
                (dict(parent=None), b"NULL device pointer (parent)"), (dict(n_filled=None), b"NULL device pointer (n_filled)")]
EMIT_CASES = ([(dict(**{k: None}), b"NULL device pointer (weights)") for k in ("child_w1", "child_b1", "child_w2", "child_b2", "elite_w1", "elite_b1", "elite_w2", "elite_b2")]
              + [(dict(child_w1=AT["elite_w1"]), b"child_w1 overlaps elite_w1"), (dict(child_b2=AT["elite_w2"] + M_ * C_ * LEN["w2"] * 4 - 4), b"child_b2 overlaps elite_w2"),
                 (dict(child_w2=AT["elite_b1"] - G_ * LEN["w2"] * 4 + 4), b"child_w2 overlaps elite_b1")])


def test_bad_arguments_are_refused_before_anything_is_dereferenced():
    """Every REM2D_E_INVALID of include/rem2d_elites.h, in the three builds, on a machine without a GPU: nothing is launched"""
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        err = L.rem2d_last_error
        calls = {"insert": (L.rem2d_elites_insert, b"elites_insert: ", INSERT_CASES), "sample": (L.rem2d_elites_sample, b"elites_sample: ", SAMPLE_CASES),
                 "emit": (L.rem2d_elites_emit, b"elites_emit: ", SAMPLE_CASES + EMIT_CASES)}
        for name, (fn, prefix, own) in calls.items():
            assert fn(None, None) == -1 and b"NULL descriptor" in err() and err().startswith(prefix)
            for kw, msg in SHAPE_CASES + SCRATCH_CASES + own:
                e = _desc(**kw)
                assert fn(C.byref(e), None) == -1 and msg in err() and err().startswith(prefix), (name, kw, err())
        assert L.rem2d_elites_scratch_bytes(None) == -1 and err().startswith(b"elites_scratch_bytes: ")
        for kw, msg in SHAPE_CASES:
            assert L.rem2d_elites_scratch_bytes(C.byref(_desc(**kw))) == -1 and msg in err(), (kw, err())
        assert L.rem2d_elites_scratch_bytes(C.byref(_desc())) == NEED
        assert L.rem2d_elites_scratch_bytes(C.byref(_desc(**{k: None for k in POINTERS}))) == NEED          # no pointer is looked at
        assert L.rem2d_elites_scratch_bytes(C.byref(_desc(bins={0: 256, 1: 256}, n_blocks=32767))) == 12 * 32767 * 65536
        # what passes: every limit itself, touching buffers, no mask, what a call does not look at -- shown through the refusal that
        # comes last, the scratch that is one byte short
        passing = [dict(max_bodies=1, d=14), dict(max_bodies=64, d=8 + 6 * 64 + 64), dict(hidden=1), dict(hidden=128), dict(d=104), dict(d=168),
                   dict(width=32, word={1: 31}), dict(n_dims=1, word={0: 7}), dict(n_dims=4, word={2: 1, 3: 2}, bins={0: 2, 1: 2, 2: 2, 3: 2}, lo={2: -3e38, 3: 3e38}, inv={2: 1e-45, 3: 3e38}),
                   dict(n_dims=1, word={1: 99}, bins={1: 0}, lo={1: nan}, inv={1: -1.0}), dict(rate_threshold=0), dict(mask=None)]
        for kw in passing:
            short = 12 * M_ * (4 if kw.get("n_dims") == 1 else C_) - 1
            for fn in (L.rem2d_elites_insert, L.rem2d_elites_sample, L.rem2d_elites_emit):
                assert fn(C.byref(_desc(scratch_bytes=short, **kw)), None) == -1 and b"scratch holds %d bytes" % short in err(), (kw, err())
        short = dict(scratch_bytes=NEED - 1)
        for kw in (dict(desc=AT["elite_desc"] + M_ * C_ * B_ * 4), dict(desc=AT["count"] - DESC_BYTES), dict(w1=AT["elite_w1"] - G_ * LEN["w1"] * 4),
                   dict(group_size=1), dict(n_children=0, parent=None, n_filled=None), dict(child_w1=None, child_b2=AT["elite_w1"])):
            assert L.rem2d_elites_insert(C.byref(_desc(**short, **kw)), None) == -1 and b"scratch holds" in err(), (kw, err())
        for kw in (dict(n_children=4), dict(n_children=2 ** 31 - 4), dict(group_size=0, desc=None, fitness=None, w1=None, cell=None, winner=None, elite_fitness=None, elite_desc=None),
                   dict(child_w1=AT["elite_w1"] + M_ * C_ * LEN["w1"] * 4), dict(child_b1=AT["elite_b1"] - G_ * LEN["b1"] * 4)):
            assert L.rem2d_elites_emit(C.byref(_desc(**short, **kw)), None) == -1 and b"scratch holds" in err(), (kw, err())
        assert L.rem2d_elites_sample(C.byref(_desc(child_w1=None, elite_w1=None, child_b2=AT["elite_w1"], **short)), None) == -1 and b"scratch holds" in err()
        big = _desc(n_blocks=32767, bins={0: 256, 1: 256}, n_children=32767, scratch_bytes=12 * 32767 * 65536 - 1)
        for k in POINTERS:
            setattr(big, k, (POINTERS.index(k) + 1) << 44)
        assert L.rem2d_elites_emit(C.byref(big), None) == -1 and b"scratch holds" in err(), err()


def test_elites_value_errors():
    """Every ValueError of the Python layer, none of which needs a GPU: they come before anything is allocated or launched"""
    import torch
    from gym_rem2d_amd import elites, evaluate, policy
    from gym_rem2d_amd.env import BatchedModular2D
    like = policy.MLPPolicy.random(8, 1, 2, n_rays=0)
    good = dict(n_blocks=2, dims=[(0, -1.0, 1.0, 4), (1, 0.0, 2.0, 3)], width=2, like=like)
    for kw, match in ((dict(n_blocks=0), "n_blocks"), (dict(width=0), "width"), (dict(width=33), "width"), (dict(like=None), "like"),
                      (dict(dims=[]), "dims"), (dict(dims=[(0, 0, 1, 2)] * 5), "dims"), (dict(dims=[(0, 0, 1)]), "dims"), (dict(dims=7), "dims"),
                      (dict(dims=[(2, 0, 1, 2)]), "word"), (dict(dims=[(-1, 0, 1, 2)]), "word"), (dict(dims=[(0.5, 0, 1, 2)]), "word"),
                      (dict(dims=[(0, 0, 1, 0)]), "bins"), (dict(dims=[(0, 0, 1, 2.5)]), "bins"), (dict(dims=[(0, 1, 1, 2)]), "lo < hi"),
                      (dict(dims=[(0, 2, 1, 2)]), "lo < hi"), (dict(dims=[(0, nan, 1, 2)]), "lo < hi"), (dict(dims=[(0, 0, inf, 2)]), "lo < hi"),
                      (dict(dims=[(0, -3e38, 3e38, 2)]), "finite positive"), (dict(dims=[(0, 0, 1, 257), (1, 0, 1, 256)]), "cells"),
                      (dict(n_blocks=32768, dims=[(0, 0, 1, 65536)]), "2\\^31")):
        with pytest.raises(ValueError, match=match):
            elites.EliteGrid(**dict(good, **kw))
    g = elites.EliteGrid(**good)
    assert g.n_cells == 12 and g.fitness.shape == (2, 12) and g.desc.shape == (2, 12, 2) and g.count.dtype == torch.int32
    assert g.w1.shape == (24, 14, 2) and g.b2.shape == (24, 1) and g.scratch.numel() * 8 >= 12 * 24 and (g.winner == -1).all()
    assert g.inv == [2.0, 1.5] and g.lo == [-1.0, 0.0] and g.n_filled.tolist() == [0, 0] and g.coverage().tolist() == [0.0, 0.0]
    g.count[1, 3], g.fitness[1, 3], g.fitness[0, 0] = 2, 4.5, 100.0
    assert g.n_filled.tolist() == [0, 1] and g.qd_score().tolist() == [0.0, 4.5] and g.coverage()[1] == 1 / 12
    assert g.elites(1).n_sets == 1 and g.elites(1).activation == like.activation
    for bad, match in ((lambda: g.elites(2), "block"), (lambda: g.elites(0), "no filled cell")):
        with pytest.raises(ValueError, match=match):
            bad()
    fit, d = torch.zeros(8, dtype=torch.float64), torch.zeros((8, 2))
    other = policy.MLPPolicy.random(8, 1, 3, n_rays=0)
    shared = policy.MLPPolicy(g.w1[:8], like.b1, like.w2, like.b2)
    indexed = policy.MLPPolicy(like.w1, like.b1, like.w2, like.b2, index=torch.arange(8))
    inside = torch.zeros(16 + 48)
    g2 = elites.EliteGrid(**good)
    g2.desc = inside[:48].view(2, 12, 2)
    cases = [
        ("MLPPolicy", lambda: g.insert(None, fit, d)), ("index", lambda: g.insert(indexed, fit, d)), ("the grid's", lambda: g.insert(other, fit, d)),
        ("must be on", lambda: g.insert(like.to("meta"), fit, d)), ("shares memory", lambda: g.insert(shared, fit, d)),
        ("float64", lambda: g.insert(like, fit.float(), d)), ("fitness", lambda: g.insert(like, torch.zeros(7, dtype=torch.float64), d)),
        ("fitness", lambda: g.insert(like, torch.zeros(16, dtype=torch.float64)[::2], d)), ("float32", lambda: g.insert(like, fit, d.double())),
        ("desc", lambda: g.insert(like, fit, torch.zeros((8, 3)))), ("desc", lambda: g.insert(like, fit, torch.zeros((8, 4))[:, ::2])),
        ("blocks", lambda: g.insert(like, fit, d, group_size=2)), ("blocks", lambda: g.insert(like, fit, d, group_size=0)),
        ("blocks", lambda: g.insert(policy.MLPPolicy.random(7, 1, 2, n_rays=0), torch.zeros(7, dtype=torch.float64), torch.zeros((7, 2)))),
        ("mask", lambda: g.insert(like, fit, d, mask=torch.zeros(8))), ("mask", lambda: g.insert(like, fit, d, mask=[1] * 8)),
        ("mask", lambda: g.insert(like, fit, d, mask=torch.zeros(7, dtype=torch.bool))),
        ("desc shares memory", lambda: g2.insert(like, fit, inside[40:56].view(8, 2))),
        ("GPU", lambda: g.insert(like, fit, d)), ("GPU", lambda: g.insert(like, fit, d, mask=torch.ones(8, dtype=torch.bool), group_size=4)),
        ("generation", lambda: g.sample(-1)), ("generation", lambda: g.sample(2 ** 32)), ("generation", lambda: g.emit(1, seed=2 ** 64)),
        ("n_children", lambda: g.sample(1, n_children=3)), ("n_children", lambda: g.sample(1, n_children=0)), ("n_children", lambda: g.emit(1, n_children=-2)),
        ("parents", lambda: g.sample(1, n_children=4, out=torch.zeros(4))), ("parents", lambda: g.sample(1, n_children=4, out=torch.zeros(2, dtype=torch.int32))),
        ("rate", lambda: g.emit(1, rate=-0.1)), ("rate", lambda: g.emit(1, rate=1.5)), ("rate", lambda: g.emit(1, rate=nan)),
        ("MLPPolicy", lambda: g.emit(1, out=g)), ("the grid's", lambda: g.emit(1, out=other)), ("shares memory", lambda: g.emit(1, out=shared)),
        ("must have 4", lambda: g.emit(1, n_children=4, out=like)), ("n_children", lambda: g.emit(1, out=policy.MLPPolicy.random(7, 1, 2, n_rays=0))),
        ("GPU", lambda: g.sample(1)), ("GPU", lambda: g.emit(1)), ("GPU", lambda: g.emit(1, n_children=8, out=like)),
    ]
    for match, bad in cases:
        with pytest.raises(ValueError, match=match):
            bad()
    # checkpoints
    g.w1[15, 3, 1] = 2.5
    state = g.state_dict()
    h = elites.EliteGrid(**good)
    h.load_state_dict(state)
    g.w1.zero_()
    assert h.w1[15, 3, 1] == 2.5 and h.count[1, 3] == 2 and h.fitness[1, 3] == 4.5 and state["w1"][15, 3, 1] == 2.5
    for bad_state, match in ((dict(state, desc=torch.zeros((2, 12, 3))), "desc"), (dict(state, count=torch.zeros((2, 12), dtype=torch.int64)), "count")):
        with pytest.raises(ValueError, match=match):
            h.load_state_dict(bad_state)
    assert h.count[1, 3] == 2                                  # (a refused state wrote nothing)
    # the loop
    env = BatchedModular2D()
    with pytest.raises(ValueError, match="EliteGrid"):
        evaluate.run_policy_map_elites(env, like, None, 1)
    with pytest.raises(ValueError, match="reset first"):
        evaluate.run_policy_map_elites(env, like, g, 1)
    env.worlds = [(None, None)]                               # (a population "in place": the checks that follow look at nothing of it)
    env.n_envs = 8
    env._autoreset = (("done",), 100)
    with pytest.raises(ValueError, match="auto-reset or streaming"):
        evaluate.run_policy_map_elites(env, like, g, 1)
    env._autoreset, env._stream_rec = None, object()
    with pytest.raises(ValueError, match="auto-reset or streaming"):
        evaluate.run_policy_map_elites(env, like, g, 1)
    env._stream_rec = None
    for args, kw, match in (((like, g, 1), dict(group_size=2), "blocks"), ((other.take([0, 1, 2]), g, 1), {}, "one weight set per creature"),
                            ((indexed, g, 1), {}, "one weight set per creature"), ((like, g, 1), dict(samples=2), "2 \\* samples")):
        with pytest.raises(ValueError, match=match):
            evaluate.run_policy_map_elites(env, *args, **kw)
    env.worlds = []


# ---------------------------------------------------------------------------------------------- what MAP-Elites is for
WALL_Y, WALL_HALF, GOAL, REACH = 1.0, 1.2, np.array([0.0, 2.0]), 0.35
ARENA = np.array([[-2.0, -1.0], [2.0, 3.0]])
TOY_SHAPES = ((14, 2), (2,), (2, 1), (1,))
TOY = dict(generations=60, S=64, sigma=0.2, bins=5)


def toy_walk(theta):
    """DESIGN.md 17's walled point-walk: from the origin to waypoint (theta_0, theta_1) and on by (theta_2, theta_3); the wall
    y = 1, |x| <= 1.2 stops the point where it is met; the walk is clipped to the arena.  -> final positions [n, 2]"""
    theta = np.asarray(theta, np.float64)
    pos = np.zeros((theta.shape[0], 2))
    stopped = np.zeros(theta.shape[0], bool)
    for leg in (theta[:, 0:2], theta[:, 2:4]):
        new = pos + leg
        with np.errstate(all="ignore"):
            s = (WALL_Y - pos[:, 1]) / (new[:, 1] - pos[:, 1])
            xs = pos[:, 0] + s * (new[:, 0] - pos[:, 0])
        cross = (pos[:, 1] < WALL_Y) != (new[:, 1] < WALL_Y)
        hit = cross & (np.abs(xs) <= WALL_HALF) & ~stopped
        new[hit] = np.stack([xs[hit], np.where(pos[hit, 1] < WALL_Y, WALL_Y - 1e-3, WALL_Y + 1e-3)], axis=1)
        new[stopped] = pos[stopped]
        stopped |= hit
        pos = np.clip(new, ARENA[0], ARENA[1])
    return pos


def toy_map_elites(seed):
    """elites_model's insert and emit around one grid of bins x bins cells over the arena, the walk's end point as the behaviour,
    minus the distance to the goal as the fitness; generation 0 is S copies of the zero policy.  The invariants are asserted after
    every generation.  -> (the goal's cell is filled, filled cells)"""
    S, bins = TOY["S"], TOY["bins"]
    cmap = QM.CellMap.of([(0, ARENA[0, 0], ARENA[1, 0], bins), (1, ARENA[0, 1], ARENA[1, 1], bins)])
    grid = QM.Grid(1, cmap.n_cells, 2, TOY_SHAPES)
    goal_cell = int(QM.cells_model(cmap, GOAL[None, :].astype(f32), [0.0])[0])
    kids = [np.zeros((S,) + s, f32) for s in TOY_SHAPES]
    for gen in range(TOY["generations"] + 1):
        if gen:
            kids = QM.emit_model(grid, S, EM.rate_threshold(1.0), TOY["sigma"], seed, gen, before=kids)[0]
        end = toy_walk(kids[0].reshape(S, -1)[:, :4])
        fitness = -np.linalg.norm(end - GOAL[None, :], axis=1)
        new, cell, winner = QM.insert_model(cmap, grid, kids, fitness, end.astype(f32), S)
        was = grid.count != 0
        assert (new.fitness[was] >= grid.fitness[was]).all()                    # no elite's fitness ever decreases
        assert (new.count >= grid.count).all() and (new.count != 0).sum() >= was.sum()   # neither do count and coverage
        now = np.flatnonzero(new.count[0] != 0)
        assert np.array_equal(QM.cells_model(cmap, new.desc[0, now], new.fitness[0, now]), now)   # every elite sits in its own cell
        assert ((winner >= 0) == (new.count != grid.count)).all()
        grid = new
    return bool(grid.count[0, goal_cell] != 0), int((grid.count != 0).sum())


def toy_es_reaches(seed, generations=200, S=64, sigma=0.2, lr=0.5):
    """DESIGN.md 17's fitness-ranked strategy on the same walk (es_model's sample / shape / update around one mean): does a child
    ever end within REACH of the goal?"""
    mean = [np.zeros((1,) + s, f32) for s in TOY_SHAPES]
    step = ES.step_for(lr, S, sigma)
    for gen in range(1, generations + 1):
        kids = ES.sample_model(mean, S, sigma, seed, gen)
        dist = np.linalg.norm(toy_walk(kids[0].reshape(S, -1)[:, :4]) - GOAL[None, :], axis=1)
        if (dist < REACH).any():
            return True
        mean = ES.update_model(mean, ES.shape_model(-dist, S), S, step, seed, gen)
    return False


def test_map_elites_does_what_it_is_for():
    """The deceptive toy, a 5 x 5 grid over the arena, S = 64, seeds 0 .. 19, 60 generations at sigma 0.2 and rate 1: the grid
    invariants hold after every generation, and the goal's cell -- behind the wall -- is filled in strictly more seeds than the
    fitness-ranked evolution strategy reaches the goal in 200 generations (DESIGN.md 18 records the counts)"""
    runs = [toy_map_elites(seed) for seed in range(20)]
    filled = sum(r[0] for r in runs)
    es = sum(toy_es_reaches(seed) for seed in range(20))
    print("seeds of 20: MAP-Elites fills the goal's cell in %d (filled cells %d .. %d of 25), fitness-ranked ES reaches the goal in %d"
          % (filled, min(r[1] for r in runs), max(r[1] for r in runs), es))
    assert filled > es
