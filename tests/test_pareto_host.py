"""Pareto ranking without a GPU (include/rem2d_pareto.h): the header's worked examples, the K = 1 reduction to the evolution
strategy's rank shaping, a host model with teeth, the header, the ctypes binding and the three libraries in agreement, the argument
checks of both entry points and the value errors of the Python layer, and the ranking doing what it is for on the deceptive toy of
tests/test_novelty_host.py.

The GPU half (tests/test_pareto_gpu.py) compares the kernels with tests/pareto_model.py bit for bit; this half makes sure that the
model is no vacuous yardstick."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import es_model as ES
import novelty_model as NM
import pareto_model as PA
import test_novelty_host as TN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
nan, inf = np.nan, np.inf


# ---------------------------------------------------------------------------------------------------- the header's examples
def test_the_headers_worked_examples():
    front, crowd, util, nf = PA.rank_model([[1, 5], [2, 4], [3, 3], [2, 2], [1, 1], [nan, 9]], 6)
    assert front.tolist() == [0, 0, 0, 1, 2, 3] and crowd.tolist() == [inf, 2.0, inf, inf, inf, 0.0]
    assert util.tolist() == [4, 1, 4, -1, -3, -5] and nf.tolist() == [3]
    local, neigh = PA.local_model(np.array([[0], [3], [4], [8]], f32), [5.0, 1.0, 7.0, 7.0], 2, 4)
    assert local.tolist() == [1.0, 0.0, 2.0, 1.0] and neigh.tolist() == [2, 2, 2, 2]
    assert PA.local_model(np.array([[0], [3], [4], [8]], f32), [5.0, 1.0, 7.0, 7.0], 2, 4, variant="high_tie")[0].tolist() == [1.0, 0.0, 1.0, 1.0]
    # no admitted row: F = 0, everyone level; blocks of one; duplicates share front and crowding
    front, crowd, util, nf = PA.rank_model([[nan, 1], [1, inf], [-inf, 0]], 3)
    assert front.tolist() == [0, 0, 0] and crowd.tolist() == [0.0] * 3 and util.tolist() == [0, 0, 0] and nf.tolist() == [0]
    front, crowd, util, nf = PA.rank_model([[1, 1], [nan, 1]], 1)
    assert front.tolist() == [0, 0] and crowd.tolist() == [inf, 0.0] and util.tolist() == [0, 0] and nf.tolist() == [1, 0]
    front, crowd, util, nf = PA.rank_model([[0, 4], [1, 3], [1, 3], [2, 2], [4, 0], [-0.0, 4]], 6)
    assert front.tolist() == [0] * 6 and crowd[1] == crowd[2] == (2 - 0) / 4 + (4 - 2) / 4 and crowd[0] == crowd[5] == inf
    assert crowd[3] == (4 - 1) / 4 + (3 - 0) / 4 and util.sum() == 0
    # an overflowing range: (above - below) / (hi - lo) = finite / inf = 0, or inf / inf = NaN, which ranks below every number
    big = 1.7e308
    front, crowd, util, nf = PA.rank_model([[-big, 3], [-1, 2], [0, 1], [1, 0], [big, -1]], 5)
    assert front.tolist() == [0] * 5 and crowd.tolist() == [inf, 0.5, 0.5, 0.5, inf] and util.tolist() == [3, -2, -2, -2, 3]
    front, crowd, util, nf = PA.rank_model([[-big, 2], [0, 1], [big, 0], [1, nan]], 4)
    assert front.tolist() == [0, 0, 0, 1] and np.isnan(crowd[1]) and crowd[[0, 2, 3]].tolist() == [inf, inf, 0.0] and util.tolist() == [2, -1, 2, -3]
    # local competition: k beyond the candidates, a block of one, a NaN fitness, a non-finite descriptor
    local, neigh = PA.local_model(np.array([[0], [1], [nan], [2], [1e19], [-1e19]], f32), [1.0, nan, 5.0, nan, 0.0, 2.0], 32, 6)
    assert neigh.tolist() == [4, 4, 0, 4, 3, 3] and np.isnan(local[2])        # (the two far rows are at an overflowing d2 from each other)
    assert local[[0, 1, 3, 4, 5]].tolist() == [3.0, 0.0, 0.0, 2.0, 3.0]
    assert PA.local_model(np.zeros((3, 2), f32), [1.0, 2.0, 3.0], 1, 1)[0].tolist() == [0.0] * 3


def test_one_objective_is_the_rank_shaping():
    """K = 1 and input that is finite or NaN: util equals es_model.shape_model, bit for bit"""
    rng = np.random.default_rng(3)
    for S, M in ((1, 5), (2, 9), (16, 4), (65, 3), (256, 2), (1024, 1)):
        for kind in ("finite", "tied", "nan"):
            v = rng.standard_normal(S * M)
            if kind != "finite":
                v = rng.integers(-2, 3, S * M).astype(np.float64)
                v[rng.random(S * M) < 0.2] = -0.0
            if kind == "nan":
                v[rng.random(S * M) < 0.3] = nan
            front, crowd, util, nf = PA.rank_model(v, S)
            assert util.dtype == np.int32 and np.array_equal(util, ES.shape_model(v, S)), (S, M, kind)
            assert (util.reshape(M, S).sum(axis=1) == 0).all() and np.abs(util).max() <= S - 1
            assert (crowd[np.isfinite(v)] == inf).all() and (crowd[np.isnan(v)] == 0.0).all()
    # an infinite word is where the two part: unadmitted here, a number there
    assert PA.rank_model([1.0, inf, 0.0], 3)[2].tolist() == [2, -2, 0] and ES.shape_model([1.0, inf, 0.0], 3).tolist() == [0, 2, -2]


# ------------------------------------------------------------------------------------------------------------------- teeth
def rank_teeth_inputs(variant):
    """4 blocks of 64 rows.  Small integers (ties, duplicate vectors) show weak domination, sort neighbours and row-ordered ties;
    the reversed sum shows on three objectives of normal values, whose three quotients do not add exactly"""
    rng = np.random.default_rng([7, PA.RANK_VARIANTS.index(variant)])
    if variant == "reverse":
        return rng.standard_normal((256, 3))
    return rng.integers(0, 4, (256, 2)).astype(np.float64)


def local_teeth_inputs():
    """4 blocks of 64 rows on a coarse grid (many equal d2, twins at distance 0) with tied fitness"""
    rng = np.random.default_rng(11)
    return rng.integers(0, 3, (256, 2)).astype(f32), rng.integers(0, 4, 256).astype(np.float64)


def variant_shares():
    shares = {}
    for v in PA.RANK_VARIANTS:
        obj = rank_teeth_inputs(v)
        right, wrong = PA.rank_model(obj, 64), PA.rank_model(obj, 64, variant=v)
        diff = np.concatenate([a != b for a, b in ((right[0], wrong[0]), (PA.bits64(right[1]), PA.bits64(wrong[1])), (right[2], wrong[2]))])
        shares[v] = float(diff.mean())
    desc, fit = local_teeth_inputs()
    right = PA.local_model(desc, fit, 5, 64)[0]
    for v in PA.LOCAL_VARIANTS:
        shares[v] = float((PA.bits64(right) != PA.bits64(PA.local_model(desc, fit, 5, 64, variant=v)[0])).mean())
    return shares


def test_the_model_has_teeth():
    """What a kernel could get wrong shows in the bits: weak domination (>= alone), the crowding's neighbours taken non-strictly,
    ties ordered by row instead of averaged, the objectives summed in reverse, the row counted among its own neighbours, a tie in
    d2 going to the higher index, <= for "beaten" """
    shares = variant_shares()
    print("share of outputs that change: %s" % ", ".join("%s %.1f %%" % (v, 100 * s) for v, s in shares.items()))
    assert set(shares) == set(PA.RANK_VARIANTS + PA.LOCAL_VARIANTS)
    for v, s in shares.items():
        assert s > 0.0, v


# -------------------------------------------------------------------------------------------- header, binding, libraries
EXPORTS = ["rem2d_pareto_abi_version", "rem2d_pareto_rank", "rem2d_pareto_local"]
OLDER_ABI = ("render", "control", "sense", "policy", "episode", "stream", "evolve", "order", "es", "novelty", "elites", "snes", "selftest")


def test_header_binding_and_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    with open(os.path.join(ROOT, "include", "rem2d_pareto.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*(?:int|int64_t)\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert declared == EXPORTS
    assert int(re.search(r"#define REM2D_PARETO_ABI_VERSION (\d+)", text).group(1)) == _lib.PARETO_ABI_VERSION == 1
    for name, value in (("MAX_OBJ", _lib.PARETO_MAX_OBJ), ("MAX_GROUP", _lib.PARETO_MAX_GROUP), ("MAX_WIDTH", _lib.PARETO_MAX_WIDTH),
                        ("MAX_K", _lib.PARETO_MAX_K)):
        assert int(re.search(r"#define REM2D_PARETO_%s (\d+)" % name, text).group(1)) == value
    assert (_lib.PARETO_MAX_OBJ, _lib.PARETO_MAX_GROUP, _lib.PARETO_MAX_WIDTH, _lib.PARETO_MAX_K) == (4, 1024, 32, 32)
    for words in ("equals that shaping bit for bit", "CPU\n * twin has no counterpart", "d2 = d2 + (t * t)", "(d2, row index)"):
        assert words in text, words
    body = re.search(r"typedef struct rem2d_pareto \{(.*?)\} rem2d_pareto;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+);", body, flags=re.M)
    assert [m[2] for m in members] == [n for n, _ in _lib.Pareto._fields_], members
    for (tname, star, name), (_, ct) in zip(members, _lib.Pareto._fields_):
        assert ct is (C.c_void_p if star else {"int32_t": C.c_int32}[tname]), name
    assert C.sizeof(_lib.Pareto) == 6 * 4 + 9 * 8
    assert [getattr(_lib.Pareto, n).offset for n, _ in _lib.Pareto._fields_] == [0, 4, 8, 12, 16, 20] + [24 + 8 * i for i in range(9)]
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(re.findall(r" T (rem2d_pareto\w*)", syms)) == sorted(EXPORTS), path
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        assert L.rem2d_pareto_abi_version() == _lib.PARETO_ABI_VERSION
        assert L.rem2d_abi_version() == 11
        for name in OLDER_ABI:                              # the older headers' versions are what they were
            assert getattr(L, "rem2d_%s_abi_version" % name)() == 1, name
        assert L.rem2d_pareto_rank.argtypes == L.rem2d_pareto_local.argtypes == [C.POINTER(_lib.Pareto), C.c_void_p]
    # the older headers know nothing of it, and rem2d.h is still ABI 11
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header == "rem2d_pareto.h":
            continue
        with open(os.path.join(ROOT, "include", header)) as f:
            other = f.read()
        for name in declared + ["REM2D_PARETO_", "rem2d_pareto"]:
            assert name not in other, (header, name)
    with open(os.path.join(ROOT, "include", "rem2d.h")) as f:
        assert "#define REM2D_ABI_VERSION 11 " in f.read()
    # the CPU twin has no counterpart
    for name in os.listdir(os.path.join(ROOT, "oracle")):
        if name.endswith((".c", ".h", ".py")):
            with open(os.path.join(ROOT, "oracle", name)) as f:
                assert "pareto" not in f.read(), name
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        entry = f.read()
    assert all('"%s"' % name in entry for name in declared)


OBJ_BYTES = 64 * 2 * 8                   # _desc's objectives: G = 64 rows of K = 2
DESC_BYTES = 64 * 8 * 4                  # its descriptors: B = 8
POINTERS = ("obj", "front", "crowd", "util", "n_fronts", "desc", "fitness", "local", "neighbours")
AT = {k: (i + 1) << 26 for i, k in enumerate(POINTERS)}


def _desc(**kw):
    """a good descriptor, 4 blocks of 16 rows; the "device pointers" are never dereferenced: the checks come first.  The buffers
    lie 64 MB apart."""
    from gym_rem2d_amd import _lib
    p = _lib.Pareto()
    p.n_rows, p.group_size, p.n_obj, p.width, p.k, p.reserved = 64, 16, 2, 8, 15, 0
    for k in POINTERS:
        setattr(p, k, AT[k])
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BOTH_CASES = [(dict(n_rows=0), b"n_rows"), (dict(n_rows=-64), b"n_rows"), (dict(group_size=0), b"group_size"),
              (dict(group_size=-16), b"group_size"), (dict(group_size=7), b"group_size"), (dict(group_size=128), b"group_size"),
              (dict(reserved=1), b"reserved"), (dict(reserved=-1), b"reserved")]
RANK_CASES = [(dict(n_obj=0), b"n_obj"), (dict(n_obj=5), b"n_obj"), (dict(n_rows=2050, group_size=1025), b"group_size"),
              (dict(n_rows=4096, group_size=2048), b"group_size"), (dict(obj=None), b"NULL device pointer (obj)")]
RANK_CASES += [(dict([(k, AT["obj"] + off)]), k.encode() + b" overlaps obj")
               for k, size in (("front", 256), ("crowd", 512), ("util", 256), ("n_fronts", 16)) for off in (0, OBJ_BYTES - 4 if size != 512 else OBJ_BYTES - 8, 8 - size)]
LOCAL_CASES = [(dict(width=0), b"width"), (dict(width=33), b"width"), (dict(k=0), b"k must be"), (dict(k=33), b"k must be"),
               (dict(desc=None), b"NULL device pointer (desc)"), (dict(fitness=None), b"NULL device pointer (fitness)"),
               (dict(local=None), b"NULL device pointer (local)"),
               (dict(local=AT["desc"]), b"local overlaps desc"), (dict(local=AT["desc"] + DESC_BYTES - 8), b"local overlaps desc"),
               (dict(local=AT["desc"] - 512 + 8), b"local overlaps desc"), (dict(local=AT["fitness"] + 504), b"local overlaps fitness"),
               (dict(local=AT["fitness"] - 504), b"local overlaps fitness"), (dict(neighbours=AT["desc"] + DESC_BYTES - 4), b"neighbours overlaps desc"),
               (dict(neighbours=AT["desc"] - 256 + 4), b"neighbours overlaps desc"), (dict(neighbours=AT["fitness"] + 508), b"neighbours overlaps fitness"),
               (dict(neighbours=AT["fitness"] - 252), b"neighbours overlaps fitness")]


def test_bad_arguments_are_refused_before_anything_is_dereferenced():
    """Every REM2D_E_INVALID of include/rem2d_pareto.h, in the three builds, on a machine without a GPU: nothing is launched"""
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        err = L.rem2d_last_error
        for fn, prefix, cases in ((L.rem2d_pareto_rank, b"pareto_rank: ", BOTH_CASES + RANK_CASES),
                                  (L.rem2d_pareto_local, b"pareto_local: ", BOTH_CASES + LOCAL_CASES)):
            assert fn(None, None) == -1 and b"NULL descriptor" in err() and err().startswith(prefix)
            for kw, msg in cases:
                p = _desc(**kw)
                assert fn(C.byref(p), None) == -1 and msg in err() and err().startswith(prefix), (prefix, kw, err())
        # what passes: every limit itself, touching buffers, absent outputs, the other call's members out of range -- shown through
        # the refusal that comes last (rank: n_fronts on obj; local: neighbours on fitness)
        for kw in (dict(n_obj=1), dict(n_obj=4, front=9 << 26), dict(group_size=1), dict(group_size=64), dict(n_rows=1024, group_size=1024, front=9 << 26),
                   dict(front=None), dict(crowd=None), dict(util=None), dict(front=None, crowd=None, util=None),
                   dict(front=AT["obj"] + OBJ_BYTES), dict(crowd=AT["obj"] - 512), dict(width=0, k=0, desc=None, fitness=None, local=None),
                   dict(n_rows=2 ** 31 - 1, group_size=1, front=None, crowd=None, util=None)):
            p = _desc(**dict(dict(n_fronts=AT["obj"] + 8), **kw))
            assert L.rem2d_pareto_rank(C.byref(p), None) == -1 and b"n_fronts overlaps obj" in err(), (kw, err())
        for kw in (dict(width=1), dict(width=32, local=9 << 26), dict(k=1), dict(k=32), dict(group_size=1), dict(group_size=64),
                   dict(n_rows=4096, group_size=2048, local=9 << 26), dict(local=AT["desc"] + DESC_BYTES), dict(local=AT["fitness"] - 512),
                   dict(n_obj=0, obj=None), dict(n_obj=9), dict(n_rows=2 ** 31 - 1, group_size=1, local=1 << 62, desc=1 << 61)):
            p = _desc(**dict(dict(neighbours=AT["fitness"] + 4), **kw))
            assert L.rem2d_pareto_local(C.byref(p), None) == -1 and b"neighbours overlaps fitness" in err(), (kw, err())


def test_pareto_value_errors():
    """Every ValueError of the Python layer, none of which needs a GPU: they come before anything is allocated or launched"""
    import torch
    from gym_rem2d_amd import evaluate, novelty, pareto, policy
    from gym_rem2d_amd.env import BatchedModular2D
    o = torch.zeros((8, 2), dtype=torch.float64)
    view = torch.zeros(64, dtype=torch.float64)
    i32, f64 = torch.int32, torch.float64
    d, fit = torch.zeros((8, 3)), torch.zeros(8, dtype=f64)
    cases = [
        ("float64", lambda: pareto.rank(o.float())), ("float64", lambda: pareto.rank(o.numpy())), (r"\[G, K\]", lambda: pareto.rank(torch.zeros((2, 2, 2), dtype=f64))),
        (r"\[G, K\]", lambda: pareto.rank(torch.zeros((0, 2), dtype=f64))), (r"\[G, K\]", lambda: pareto.rank(torch.zeros((8, 4), dtype=f64)[:, ::2])),
        ("objectives, not", lambda: pareto.rank(torch.zeros((8, 5), dtype=f64))), ("objectives, not", lambda: pareto.rank(torch.zeros((8, 0), dtype=f64))),
        ("group_size", lambda: pareto.rank(o, group_size=3)), ("group_size", lambda: pareto.rank(o, group_size=0)),
        ("group_size", lambda: pareto.rank(torch.zeros((2048, 1), dtype=f64))), ("group_size", lambda: pareto.rank(torch.zeros(4096, dtype=f64), group_size=2048)),
        ("four tensors", lambda: pareto.rank(o, out=(None, None, None))), ("out.front", lambda: pareto.rank(o, out=(torch.zeros(8), None, None, None))),
        ("out.front", lambda: pareto.rank(o, out=(torch.zeros(9, dtype=i32), None, None, None))),
        ("out.crowd", lambda: pareto.rank(o, out=(None, torch.zeros(8), None, None))), ("out.util", lambda: pareto.rank(o, out=(None, None, torch.zeros(16, dtype=i32)[::2], None))),
        ("out.n_fronts", lambda: pareto.rank(o, group_size=4, out=(None, None, None, torch.zeros(8, dtype=i32)))),
        ("out.util", lambda: pareto.rank(o, out=(None, None, torch.zeros(8, dtype=i32, device="meta"), None))),
        ("shares memory", lambda: pareto.rank(view[:16].view(8, 2), out=(None, view[15:23], None, None))),
        ("shares memory", lambda: pareto.rank(view[8:24].view(8, 2), out=(view[4:8].view(i32), None, view[22:26].view(i32), None))),
        ("GPU", lambda: pareto.rank(o)), ("GPU", lambda: pareto.rank(torch.zeros(8, dtype=f64), group_size=4, out=(None, None, torch.zeros(8, dtype=i32), None))),
        ("float32", lambda: pareto.local_competition(d.double(), fit)), ("float32", lambda: pareto.local_competition(d.numpy(), fit)),
        (r"\[G, B\]", lambda: pareto.local_competition(torch.zeros(8), fit)), (r"\[G, B\]", lambda: pareto.local_competition(torch.zeros((8, 33)), fit)),
        (r"\[G, B\]", lambda: pareto.local_competition(torch.zeros((8, 0)), fit)), (r"\[G, B\]", lambda: pareto.local_competition(torch.zeros((0, 3)), fit[:0])),
        (r"\[G, B\]", lambda: pareto.local_competition(torch.zeros((8, 6))[:, ::2], fit)),
        ("fitness", lambda: pareto.local_competition(d, fit.float())), ("fitness", lambda: pareto.local_competition(d, torch.zeros(9, dtype=f64))),
        ("fitness", lambda: pareto.local_competition(d, torch.zeros(16, dtype=f64)[::2])), ("fitness", lambda: pareto.local_competition(d, fit.to("meta"))),
        ("fitness", lambda: pareto.local_competition(d, [0.0] * 8)),
        ("k must be", lambda: pareto.local_competition(d, fit, k=0)), ("k must be", lambda: pareto.local_competition(d, fit, k=33)),
        ("group_size", lambda: pareto.local_competition(d, fit, group_size=3)), ("group_size", lambda: pareto.local_competition(d, fit, group_size=0)),
        ("out must be", lambda: pareto.local_competition(d, fit, out=torch.zeros(8))), ("out must be", lambda: pareto.local_competition(d, fit, out=torch.zeros(9, dtype=f64))),
        ("shares memory with desc", lambda: pareto.local_competition(view[:12].view(torch.float32).view(8, 3), fit, out=view[11:19])),
        ("shares memory with fitness", lambda: pareto.local_competition(d, view[:8], out=view[7:15])),
        ("GPU", lambda: pareto.local_competition(d, fit)), ("GPU", lambda: pareto.local_competition(d, fit, k=32, group_size=1, out=torch.zeros(8, dtype=f64))),
    ]
    for match, bad in cases:
        with pytest.raises(ValueError, match=match):
            bad()
    # the loops
    env = BatchedModular2D()
    a = novelty.NoveltyArchive(2, 4, 8)
    mean, pop = policy.MLPPolicy.random(2, 16, 32), policy.MLPPolicy.random(8, 16, 32)
    loops = {"run_policy_pareto_es": lambda **kw: evaluate.run_policy_pareto_es(env, mean, 1, kw.pop("archive", a), **dict(dict(group_size=4), **kw)),
             "run_policy_nslc": lambda **kw: evaluate.run_policy_nslc(env, pop, 1, kw.pop("archive", a), **dict(dict(group_size=4), **kw))}
    for name, loop in loops.items():
        with pytest.raises(ValueError, match="on_error"):
            loop(on_error="fallback")
        with pytest.raises(ValueError, match=name + ": no population in place"):
            loop()
        env.worlds, env.n_envs = [(None, None)], 8        # (a population "in place": the checks that follow look at nothing of it)
        try:
            env._autoreset = (("done",), 100)
            with pytest.raises(ValueError, match=name + ".*auto-reset or streaming"):
                loop()
            env._autoreset, env._stream_rec = None, object()
            with pytest.raises(ValueError, match=name + ".*auto-reset or streaming"):
                loop()
            env._stream_rec = None
            for kw in (dict(group_size=3), dict(group_size=0), dict(group_size=16)) + ((dict(group_size=8), dict(group_size=2)) if "es" in name else ()):
                with pytest.raises(ValueError, match=name + ".*group_size"):
                    loop(**kw)
            for kw in (dict(samples=3), dict(archive=novelty.NoveltyArchive(3, 4, 8)), dict(archive=novelty.NoveltyArchive(2, 4, 6))):
                with pytest.raises(ValueError, match=name + ": the archive must have 2 blocks of width"):
                    loop(**kw)
        finally:
            env.worlds, env._autoreset, env._stream_rec = [], None, None
    with pytest.raises(ValueError, match="even"):
        env.worlds, env.n_envs = [(None, None)], 6
        try:
            evaluate.run_policy_pareto_es(env, mean, 1, a, group_size=3)
        finally:
            env.worlds = []
    with pytest.raises(ValueError, match="run_policy_nslc: 8 creatures and 2 weight sets"):
        env.worlds, env.n_envs = [(None, None)], 8
        try:
            evaluate.run_policy_nslc(env, mean, 1, a, group_size=4)
        finally:
            env.worlds = []


# -------------------------------------------------------------------------------------------------- what the ranking is for
def pareto_search(seed, generations=200, S=64, sigma=0.2, lr=0.5, k=10, cap=256, rate=0.1):
    """test_novelty_host.toy_search with the Pareto utility over (-distance, novelty) in place of the weighted sum of ranks:
    -> the first generation at which a child ends within REACH of the goal, or None"""
    mean = [np.zeros(s, f32) for s in ((1, 14, 2), (1, 2), (1, 2, 1), (1, 1))]
    archive, total = np.zeros((1, cap, 2), f32), np.zeros(1, np.int64)
    step = ES.step_for(lr, S, sigma)
    for gen in range(1, generations + 1):
        kids = ES.sample_model(mean, S, sigma, seed, gen)
        end = TN.toy_walk(kids[0].reshape(S, -1)[:, :4])
        dist = np.linalg.norm(end - TN.GOAL[None, :], axis=1)
        if (dist < TN.REACH).any():
            return gen
        beh = end.astype(f32)
        nov = NM.score_model(beh, S, k, archive, total)
        archive, total, _ = NM.add_model(beh, S, archive, total, gen, seed, NM.rate_threshold(rate))
        util = PA.rank_model(np.stack([-dist, nov], axis=1), S)[2]
        mean = ES.update_model(mean, util, S, step, seed, gen)
    return None


def test_pareto_ranking_does_what_it_is_for():
    """The deceptive toy of test_novelty_host, S = 64, seeds 0 .. 19, 200 generations: the sum of the two ranks, weights (1, 1), is
    held by its fitness half and walks to the wall; the Pareto utility over (-distance, novelty) finds the way round in strictly
    more seeds (DESIGN.md 20 records the counts: 10 against 0)"""
    pareto = [pareto_search(seed) for seed in range(20)]
    mixed = sum(TN.toy_search(seed, (1, 1)) is not None for seed in range(20))
    reached = sum(g is not None for g in pareto)
    print("seeds of 20 that reach the goal: Pareto utility %d (generations %s), the (1, 1) sum of ranks %d"
          % (reached, [g for g in pareto if g is not None], mixed))
    assert reached > mixed
