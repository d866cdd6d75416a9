"""Behavioural novelty without a GPU (include/rem2d_novelty.h): a host model with teeth, the header's worked examples, the header,
the ctypes binding and the three libraries in agreement, the argument checks of the four entry points and the value errors of the
Python layer, the describe rule on the oracle's trajectories, and novelty search doing what it is for on a deceptive toy.

The GPU half (tests/test_novelty_gpu.py) compares the kernels with tests/novelty_model.py bit for bit; this half makes sure that the
model is no vacuous yardstick."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import control_model as CM
import es_model as ES
import novelty_model as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
nan, inf = np.nan, np.inf
CONT = 1


# ------------------------------------------------------------------------------------------------------------------- teeth
def teeth_inputs(B, wide_range):
    """2 blocks of 64 rows and 16 archive entries, 12 live.  wide_range: the rows' scales spread over 36 decades, so that a
    row's nearest distances span more than the 29 bits that binary64 has beyond a binary32 word and no longer add exactly"""
    rng = np.random.default_rng([B, int(wide_range)])
    desc = rng.standard_normal((128, B))
    arch = rng.standard_normal((2, 16, B))
    if wide_range:
        desc *= 10.0 ** rng.uniform(-18, 18, (128, 1))
        arch *= 10.0 ** rng.uniform(-18, 18, (2, 16, 1))
    return desc.astype(f32), arch.astype(f32), np.array([12, 40], np.int64)


def variant_shares(B):
    shares = {}
    for v in NM.VARIANTS:
        desc, arch, total = teeth_inputs(B, v == "descending")
        k = 32 if v == "descending" else 15                 # (the more roots, the wider their span)
        right = NM.score_model(desc, 64, k, arch, total)
        assert np.isfinite(right).all() and (right > 0).all()
        wrong = NM.score_model(desc, 64, k, arch, total, variant=v)
        shares[v] = float((NM.bits64(right) != NM.bits64(wrong)).mean())
    return shares


@pytest.mark.parametrize("B", [8, 32])
def test_the_model_has_teeth(B):
    """What a kernel could get wrong shows in the bits of the score: the words summed in reverse, a binary64 accumulator, a fused
    multiply-add, the row counted among its own neighbours, the archive left out, the roots summed from the largest"""
    shares = variant_shares(B)
    print("B = %d: share of scores that change: %s" % (B, ", ".join("%s %.1f %%" % (v, 100 * s) for v, s in shares.items())))
    for v, s in shares.items():
        assert s > 0.0, v
    assert shares["self"] == 1.0 and shares["no_archive"] > 0.5 and shares["reverse"] > 0.3 and shares["acc64"] > 0.3 and shares["fma"] > 0.3


def test_numpy_sqrt_on_float32_is_correctly_rounded():
    """the model's roots: binary64 sqrt rounded once to binary32 is the correctly rounded binary32 root (53 >= 2 * 24 + 2)"""
    vals = [NM.sq_dists(*(lambda d: (d, d))(teeth_inputs(B, w)[0])).ravel() for B in (8, 32) for w in (False, True)]
    vals.append(np.array([0.0, 1e-45, 1.1754942e-38, 1.1754944e-38, 2.0, 3.0, 3.4028235e38, 0.99999994, 1.0000001], f32))
    v = np.concatenate(vals)
    v = v[np.isfinite(v)]
    assert len(v) > 60000 and v.dtype == f32
    got = np.sqrt(v)
    assert got.dtype == f32 and np.array_equal(got.view(np.uint32), np.sqrt(v.astype(np.float64)).astype(f32).view(np.uint32))


# ---------------------------------------------------------------------------------------------------- the header's examples
def test_the_headers_worked_examples():
    desc = np.array([[0.0], [3.0], [4.0], [8.0]], f32)
    got = NM.score_model(desc, 4, 2, np.array([[[10.0]]], f32), [1])
    assert got.tolist() == [3.5, 2.0, 2.5, 3.0]
    # without the entry (total 0: not live), k beyond the candidates, and a block of one
    assert NM.score_model(desc, 4, 2, np.array([[[10.0]]], f32), [0]).tolist() == [3.5, 2.0, 2.5, 4.5]
    assert NM.score_model(desc, 4, 32).tolist() == [5.0, 3.0, 3.0, (8 + 5 + 4) / 3.0]
    assert NM.score_model(desc, 1, 3).tolist() == [0.0] * 4
    # duplicates are excluded by index: the twin at distance 0 counts
    assert NM.score_model(np.array([[1.0], [1.0], [2.0]], f32), 3, 1).tolist() == [0.0, 0.0, 1.0]
    # a NaN query scores NaN and is nobody's neighbour; an overflowing distance is ignored
    got = NM.score_model(np.array([[nan], [1.0], [3.0], [inf], [-3e38]], f32), 5, 2)
    assert np.isnan(got[0]) and np.isnan(got[3]) and got[1] == 2.0 and got[2] == 2.0 and got[4] == 0.0
    every = 2 ** 32
    rows = np.arange(8, dtype=f32).reshape(8, 1)
    # the ring wraps: cap 3, total 2, rows 5 and 6
    a, t, took = NM.add_model(rows, 8, np.full((1, 3, 1), -1.0, f32), [2], 0, 0, every, mask=[0, 0, 0, 0, 0, 1, 1, 0])
    assert a.ravel().tolist() == [6.0, -1.0, 5.0] and t.tolist() == [4] and took.sum() == 2
    # more than cap rows: only the last cap of them are written
    a, t, took = NM.add_model(rows, 8, np.full((1, 3, 1), -1.0, f32), [1], 0, 0, every, mask=[0, 1, 1, 1, 1, 1, 0, 0])
    assert a.ravel().tolist() == [3.0, 4.0, 5.0] and t.tolist() == [6]
    # cap 0: total still counts; threshold 0: nobody; non-finite rows never
    a, t, _ = NM.add_model(rows, 4, np.zeros((2, 0, 1), f32), [0, 7], 0, 0, every)
    assert a.size == 0 and t.tolist() == [4, 11]
    assert NM.add_model(rows, 8, np.zeros((1, 3, 1), f32), [0], 0, 0, 0)[1].tolist() == [0]
    bad = rows.copy()
    bad[2], bad[5] = nan, -inf
    assert NM.add_model(bad, 8, np.zeros((1, 3, 1), f32), [0], 0, 0, every)[2].tolist() == [1, 1, 0, 1, 1, 0, 1, 1]
    # the draw: about the rate, another generation or seed gives other rows, domain 9
    many = np.zeros((4096, 1), f32)
    took = [NM.admitted(many, g, s, NM.rate_threshold(0.3)) for g, s in ((1, 0), (2, 0), (1, 1))]
    assert all(0.27 < t.mean() < 0.33 for t in took) and (took[0] != took[1]).any() and (took[0] != took[2]).any()
    assert NM.NOVELTY_DOMAIN == 9 and NM.NOVELTY_DOMAIN > ES.ES_DOMAIN0 + 4
    assert NM.rate_threshold(0.0) == 0 and NM.rate_threshold(1.0) == 2 ** 32 and NM.rate_threshold(0.02) == 85899345


# -------------------------------------------------------------------------------------------- header, binding, libraries
EXPORTS = ["rem2d_novelty_abi_version", "rem2d_worlds_describe", "rem2d_novelty_score", "rem2d_novelty_add", "rem2d_novelty_step"]


def test_header_binding_and_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    with open(os.path.join(ROOT, "include", "rem2d_novelty.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*(?:int|int64_t)\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert declared == EXPORTS
    assert int(re.search(r"#define REM2D_NOVELTY_ABI_VERSION (\d+)", text).group(1)) == _lib.NOVELTY_ABI_VERSION == 1
    for name, value in (("MAX_WIDTH", _lib.NOVELTY_MAX_WIDTH), ("MAX_K", _lib.NOVELTY_MAX_K), ("MAX_SAMPLES", _lib.NOVELTY_MAX_SAMPLES)):
        assert int(re.search(r"#define REM2D_NOVELTY_%s (\d+)" % name, text).group(1)) == value
    for const in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "generation, 9)", "CPU twin has no counterpart"):
        assert const in text, const
    body = re.search(r"typedef struct rem2d_novelty \{(.*?)\} rem2d_novelty;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+);", body, flags=re.M)
    assert [m[2] for m in members] == [n for n, _ in _lib.Novelty._fields_], members
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    for (tname, star, name), (_, ct) in zip(members, _lib.Novelty._fields_):
        assert ct is (C.c_void_p if star else ctype[tname]), name
    assert C.sizeof(_lib.Novelty) == 6 * 4 + 2 * 8 + 5 * 8 + 8
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in declared:
            assert (" T " + name) in syms, (path, name)
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        assert L.rem2d_novelty_abi_version() == _lib.NOVELTY_ABI_VERSION
        assert L.rem2d_abi_version() == 11 and L.rem2d_es_abi_version() == 1 and L.rem2d_evolve_abi_version() == 1
        assert L.rem2d_worlds_describe.argtypes == [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    # the older headers know nothing of it
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header == "rem2d_novelty.h":
            continue
        with open(os.path.join(ROOT, "include", header)) as f:
            other = f.read()
        for name in declared + ["REM2D_NOVELTY_", "rem2d_novelty"]:
            assert name not in other, (header, name)


POINTERS = ("desc", "archive", "total", "novelty", "add_mask")
DESC_BYTES = 64 * 8 * 4                 # _desc's descriptors: G = 64 rows of B = 8
ARCHIVE_BYTES = 4 * 10 * 8 * 4          # its archive: M = 4 blocks of cap = 10


def _desc(**kw):
    """a good descriptor, 4 blocks of 16 rows of 8 words; the "device pointers" are never dereferenced: the checks come first.
    The buffers lie 64 MB apart."""
    from gym_rem2d_amd import _lib
    n = _lib.Novelty()
    n.width, n.n_rows, n.group_size, n.k, n.capacity = 8, 64, 16, 15, 10
    n.generation, n.seed, n.add_threshold, n.reserved = 3, 2 ** 64 - 1, 2 ** 32, 0
    for i, k in enumerate(POINTERS):
        setattr(n, k, (i + 1) << 26)
    for k, v in kw.items():
        setattr(n, k, v)
    return n


SHAPE_CASES = [(dict(width=0), b"width"), (dict(width=33), b"width"), (dict(n_rows=0), b"n_rows"), (dict(n_rows=-64), b"n_rows"),
               (dict(group_size=0), b"group_size"), (dict(group_size=-16), b"group_size"), (dict(group_size=7), b"group_size"),
               (dict(group_size=128), b"group_size"), (dict(k=0), b"k must be"), (dict(k=33), b"k must be"), (dict(capacity=-1), b"capacity"),
               (dict(add_threshold=2 ** 32 + 1), b"add_threshold"), (dict(add_threshold=2 ** 64 - 1), b"add_threshold"),
               (dict(reserved=1), b"reserved"), (dict(reserved=-1), b"reserved"), (dict(desc=None), b"NULL device pointer (desc)"),
               (dict(total=None), b"NULL device pointer (total)"), (dict(archive=None), b"NULL device pointer (archive)"),
               (dict(archive=1 << 26), b"archive overlaps desc"), (dict(archive=(1 << 26) + DESC_BYTES - 4), b"archive overlaps desc"),
               (dict(archive=(1 << 26) - ARCHIVE_BYTES + 4), b"archive overlaps desc")]
SCORE_CASES = [(dict(novelty=None), b"NULL device pointer (novelty)"), (dict(novelty=1 << 26), b"novelty overlaps desc"),
               (dict(novelty=(1 << 26) + DESC_BYTES - 8), b"novelty overlaps desc"), (dict(novelty=(1 << 26) - 64 * 8 + 8), b"novelty overlaps desc")]


def test_bad_arguments_are_refused_before_anything_is_dereferenced():
    """Every REM2D_E_INVALID of include/rem2d_novelty.h, in the three builds, on a machine without a GPU: nothing is launched"""
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        err = L.rem2d_last_error
        calls = {"score": (L.rem2d_novelty_score, b"novelty_score: "), "add": (L.rem2d_novelty_add, b"novelty_add: "),
                 "step": (L.rem2d_novelty_step, b"novelty_step: ")}
        for name, (fn, prefix) in calls.items():
            assert fn(None, None) == -1 and b"NULL descriptor" in err() and err().startswith(prefix)
            for kw, msg in SHAPE_CASES + (SCORE_CASES if name != "add" else []):
                n = _desc(**kw)
                assert fn(C.byref(n), None) == -1 and msg in err() and err().startswith(prefix), (name, kw, err())
        # what passes: every limit itself, touching buffers, no archive where cap is 0, no mask, no novelty for the add alone --
        # shown through the refusal that comes last (score: novelty on desc; add: the archive on desc)
        for kw in (dict(width=1), dict(width=32, archive=7 << 26), dict(k=1), dict(k=32), dict(group_size=1), dict(group_size=64),
                   dict(capacity=0, archive=None), dict(add_mask=None), dict(add_threshold=0), dict(archive=(1 << 26) + DESC_BYTES),
                   dict(archive=(1 << 26) - ARCHIVE_BYTES), dict(n_rows=2 ** 31 - 1, group_size=1, archive=1 << 62, capacity=0)):
            n = _desc(novelty=1 << 26, **kw)
            assert L.rem2d_novelty_score(C.byref(n), None) == -1 and b"novelty overlaps desc" in err(), (kw, err())
            assert L.rem2d_novelty_step(C.byref(n), None) == -1 and b"novelty overlaps desc" in err(), (kw, err())
        for kw in (dict(novelty=None), dict(novelty=1 << 26), dict(add_mask=None), dict(width=32), dict(k=32)):
            n = _desc(capacity=1, archive=(1 << 26) + 8, **kw)
            assert L.rem2d_novelty_add(C.byref(n), None) == -1 and b"archive overlaps desc" in err(), (kw, err())
        # describe: its own two refusals, then observe's, before any world is looked at
        fn = L.rem2d_worlds_describe
        one = (C.c_void_p * 1)(None)
        out = C.c_void_p(1 << 26)
        for args, msg in (((one, 1, 0, 4, out, 8), b"period"), ((one, 1, -3, 4, out, 8), b"period"), ((one, 1, 1, 0, out, 8), b"n_samples"),
                          ((one, 1, 1, 17, out, 8), b"n_samples"), ((None, 1, 1, 4, out, 8), b"no worlds"), ((one, 0, 1, 4, out, 8), b"no worlds"),
                          ((one, 1, 1, 4, None, 8), b"NULL device pointer"), ((one, 1, 1, 4, out, -1), b"negative row count"),
                          ((one, 1, 1, 16, out, 8), b"world 0 is NULL"), ((one, 1, 2 ** 31 - 1, 1, out, 0), b"world 0 is NULL")):
            assert fn(*args, None) == -1 and msg in err() and err().startswith(b"describe: "), (args[1:4], err())


def test_novelty_value_errors():
    """Every ValueError of the Python layer, none of which needs a GPU: they come before anything is allocated or launched"""
    import torch
    from gym_rem2d_amd import evaluate, novelty, policy
    from gym_rem2d_amd.env import BatchedModular2D
    for kw, match in ((dict(n_blocks=0), "n_blocks"), (dict(capacity=-1), "capacity"), (dict(width=0), "width"), (dict(width=33), "width")):
        with pytest.raises(ValueError, match=match):
            novelty.NoveltyArchive(**dict(dict(n_blocks=2, capacity=4, width=3), **kw))
    a = novelty.NoveltyArchive(2, 4, 3)
    assert a.entries.shape == (2, 4, 3) and a.entries.dtype == torch.float32 and a.total.dtype == torch.int64 and a.total.tolist() == [0, 0]
    d = torch.zeros((8, 3))
    view = torch.zeros(8 * 3 + 2 * 4 * 3)
    inside = novelty.NoveltyArchive(2, 4, 3)
    inside.entries = view[:24].view(2, 4, 3)
    cases = [
        ("float32", lambda: a.score(d.double())), ("float32", lambda: a.score(d.numpy())), (r"\[G, 3\]", lambda: a.score(torch.zeros((8, 4)))),
        (r"\[G, 3\]", lambda: a.score(torch.zeros(24))), (r"\[G, 3\]", lambda: a.score(torch.zeros((8, 6))[:, ::2])),
        (r"\[G, 3\]", lambda: a.score(torch.zeros((0, 3)))), ("desc must be on", lambda: a.score(d.to("meta"))),
        ("blocks", lambda: a.score(torch.zeros((7, 3)))), ("blocks", lambda: a.score(d, group_size=2)), ("blocks", lambda: a.score(d, group_size=0)),
        ("blocks", lambda: a.add(d, 1, group_size=8)), ("k must be", lambda: a.score(d, k=0)), ("k must be", lambda: a.step(d, 1, k=33)),
        ("generation", lambda: a.add(d, -1)), ("generation", lambda: a.add(d, 2 ** 32)), ("generation", lambda: a.step(d, 1, seed=2 ** 64)),
        ("rate", lambda: a.add(d, 1, rate=-0.1)), ("rate", lambda: a.add(d, 1, rate=1.5)), ("rate", lambda: a.step(d, 1, rate=float("nan"))),
        ("mask", lambda: a.add(d, 1, mask=torch.zeros(8))), ("mask", lambda: a.add(d, 1, mask=[1] * 8)),
        ("mask", lambda: a.add(d, 1, mask=torch.zeros(7, dtype=torch.bool))), ("mask", lambda: a.step(d, 1, mask=torch.zeros(16, dtype=torch.uint8)[::2])),
        ("out", lambda: a.score(d, out=torch.zeros(8))), ("out", lambda: a.score(d, out=torch.zeros(9, dtype=torch.float64))),
        ("out", lambda: a.step(d, 1, out=torch.zeros(16, dtype=torch.float64)[::2])),
        ("shares memory", lambda: inside.score(view[16:40].view(8, 3))),
        ("shares memory", lambda: a.score(view[:24].view(8, 3), out=view[20:36].view(torch.float64))),
        ("GPU", lambda: a.score(d)), ("GPU", lambda: a.add(d, 1)), ("GPU", lambda: a.step(d, 1, out=torch.zeros(8, dtype=torch.float64))),
        ("GPU", lambda: a.add(d, 1, mask=torch.ones(8, dtype=torch.bool), rate=1.0)),
    ]
    for match, bad in cases:
        with pytest.raises(ValueError, match=match):
            bad()
    # checkpoints
    a.entries[1, 2, 0], a.total[1] = 5.0, 9
    state = a.state_dict()
    b = novelty.NoveltyArchive(2, 4, 3)
    b.load_state_dict(state)
    a.entries.zero_()
    assert b.entries[1, 2, 0] == 5.0 and b.total.tolist() == [0, 9] and state["entries"][1, 2, 0] == 5.0
    for bad_state, match in ((dict(state, entries=torch.zeros((2, 4, 4))), "entries"), (dict(state, total=torch.zeros(2, dtype=torch.int32)), "total")):
        with pytest.raises(ValueError, match=match):
            b.load_state_dict(bad_state)
    # the env and the loops
    env = BatchedModular2D()
    assert env.behaviour is None
    env.set_descriptor(None)
    with pytest.raises(ValueError, match="reset first"):
        env.set_descriptor(5, 4)
    with pytest.raises(ValueError, match="set_descriptor first"):
        env.describe()
    with pytest.raises(ValueError, match="reset first"):
        evaluate.run_behaviour_episode(env, 5, 4)
    with pytest.raises(ValueError, match="on_error"):
        evaluate.run_behaviour_episode(env, 5, 4, on_error="fallback")
    with pytest.raises(ValueError, match="reset first"):
        evaluate.run_policy_nses(env, policy.MLPPolicy.random(3, 16, 32), 1, a, group_size=2)
    env.worlds = [(None, None)]                               # (a population "in place": the checks that follow look at nothing of it)
    for args, match in (((5, 0), "samples"), ((5, 17), "samples"), ((5, None), "samples"), ((0, 4), "period"), ((2 ** 31, 4), "period")):
        with pytest.raises(ValueError, match=match):
            env.set_descriptor(*args)
    env._autoreset = (("done",), 100)
    with pytest.raises(ValueError, match="auto-reset or streaming"):
        env.set_descriptor(5, 4)
    env._autoreset, env._stream_rec = None, object()
    with pytest.raises(ValueError, match="auto-reset or streaming"):
        env.set_descriptor(5, 4)
    env._stream_rec = None
    env._descriptor = (5, 4, None)
    env._autoreset = (("done",), 100)
    with pytest.raises(ValueError, match="auto-reset or streaming"):
        env.describe()
    env.worlds = []


# ------------------------------------------------------------------------------------------ the describe rule, on the oracle
def oracle_rows(oracle, pop="lsystem", n_steps=120):
    """per lane bucket: px, py float32 [n_steps + 1, N] of the root, frozen int [n_steps + 1, N], from the oracle's closed-loop
    run (shared with the control tests) and the step's own bookkeeping rule (NM.episode_words)"""
    out = []
    for run in CM.closed_loop_run(oracle, pop, CONT):
        obs = np.stack([o[:, :2] for o in run["obs"][:n_steps + 1]])
        out.append((obs[:, :, 0], obs[:, :, 1], NM.episode_words(obs[:, :, 0])))
    return out


def test_describe_model_on_the_oracle(oracle):
    """The rule of rem2d_worlds_describe on the oracle's own closed-loop trajectories (lsystem, 120 steps): called every step and
    called every `period` steps, a creature's rows agree on every slot below its current one, and every slot below it holds the root
    position at step (k + 1) * period; a creature that ends early keeps its row from then on.  No word had to be forged: 10 of the
    119 creatures end between steps 61 and 90, 80 last beyond step 112."""
    period, K, n = 7, 16, 120
    early = lasting = 0
    for px, py, frozen in oracle_rows(oracle, n_steps=n):
        N = px.shape[1]
        dense, sparse = np.full((N, 2 * K), -7.0, f32), np.full((N, 2 * K), -7.0, f32)
        end = np.where(frozen.any(axis=0), frozen.argmax(axis=0), n + 1)        # the first call that finds the creature over
        early += int((end <= (K - 1) * period).sum())
        lasting += int((end > K * period).sum())
        for t in range(n + 1):
            steps = np.full(N, t)
            before = dense.copy()
            NM.describe_update(dense, steps, frozen[t], px[t], py[t], period, K)
            assert np.array_equal(dense[frozen[t] != 0], before[frozen[t] != 0])
            if t % period == 0:
                NM.describe_update(sparse, steps, frozen[t], px[t], py[t], period, K)
            lastrun = np.minimum(t, end - 1)                                   # the last step at which a call recorded the creature
            for e in range(N):
                cur = min(K, int(lastrun[e]) // period)                         # slots k < cur: (k + 1) * period <= lastrun
                assert np.array_equal(dense[e, :2 * cur], sparse[e, :2 * cur]), (t, e)
                for k in range(cur):
                    assert dense[e, 2 * k] == px[(k + 1) * period, e] and dense[e, 2 * k + 1] == py[(k + 1) * period, e]
                if t == 0:
                    assert (dense[e, 0::2] == px[0, e]).all() and (dense[e, 1::2] == py[0, e]).all()
        # an early end carries the last recorded position forward, in both cadences
        for e in np.flatnonzero(end <= K * period):
            last_dense, last_sparse = end[e] - 1, ((end[e] - 1) // period) * period
            assert dense[e, -2] == px[last_dense, e] and sparse[e, -2] == px[last_sparse, e]
    print("describe on the oracle: %d creatures end before the last sample, %d last beyond it" % (early, lasting))
    assert early >= 1 and lasting >= 1


# ------------------------------------------------------------------------------------------------- what novelty is for
WALL_Y, WALL_HALF, GOAL, REACH = 1.0, 1.2, np.array([0.0, 2.0]), 0.35
ARENA = np.array([[-2.0, -1.0], [2.0, 3.0]])                # the walk is clipped to this box: there is no running away for novelty


def toy_walk(theta):
    """A point walks from the origin to waypoint (theta_0, theta_1) and on by (theta_2, theta_3); the wall y = 1, |x| <= 1.2 stops it
    where it is met.  -> final positions [n, 2].  The goal (0, 2) lies straight behind the wall: walking at it ends under the wall
    at distance 1, and every way round first leads away from the goal."""
    theta = np.asarray(theta, np.float64)
    pos = np.zeros((theta.shape[0], 2))
    stopped = np.zeros(theta.shape[0], bool)
    for leg in (theta[:, 0:2], theta[:, 2:4]):
        new = pos + leg
        with np.errstate(all="ignore"):
            s = (WALL_Y - pos[:, 1]) / (new[:, 1] - pos[:, 1])
        cross = (pos[:, 1] < WALL_Y) != (new[:, 1] < WALL_Y)
        xs = pos[:, 0] + s * (new[:, 0] - pos[:, 0])
        hit = cross & (np.abs(xs) <= WALL_HALF) & ~stopped
        new[hit] = np.stack([xs[hit], np.where(pos[hit, 1] < WALL_Y, WALL_Y - 1e-3, WALL_Y + 1e-3)], axis=1)
        new[stopped] = pos[stopped]
        stopped |= hit
        pos = np.clip(new, ARENA[0], ARENA[1])
    return pos


def toy_search(seed, weights, generations=200, S=64, sigma=0.2, lr=0.5, k=10, cap=256, rate=0.1):
    """es_model's sample / shape / update around one mean, the walk's end point as the behaviour, novelty_model's score and add:
    -> the first generation at which a child ends within REACH of the goal, or None"""
    mean = [np.zeros(s, f32) for s in ((1, 14, 2), (1, 2), (1, 2, 1), (1, 1))]
    archive, total = np.zeros((1, cap, 2), f32), np.zeros(1, np.int64)
    step = ES.step_for(lr, S, sigma)
    for gen in range(1, generations + 1):
        kids = ES.sample_model(mean, S, sigma, seed, gen)
        end = toy_walk(kids[0].reshape(S, -1)[:, :4])
        dist = np.linalg.norm(end - GOAL[None, :], axis=1)
        if (dist < REACH).any():
            return gen
        beh = end.astype(f32)
        nov = NM.score_model(beh, S, k, archive, total)
        archive, total, _ = NM.add_model(beh, S, archive, total, gen, seed, NM.rate_threshold(rate))
        util = NM.combine_util(ES.shape_model(-dist, S), ES.shape_model(nov, S), weights)
        mean = ES.update_model(mean, util, S, step, seed, gen)
    return None


def test_novelty_search_does_what_it_is_for():
    """The deceptive toy, S = 64, seeds 0 .. 19, 200 generations: fitness ranks alone walk to the wall and stay there; novelty ranks
    find the way round in strictly more seeds (DESIGN.md 17 records the counts)"""
    reached = {w: sum(toy_search(seed, w) is not None for seed in range(20)) for w in ((1, 0), (0, 1), (1, 1))}
    print("seeds of 20 that reach the goal: fitness alone %d, novelty alone %d, both %d" % (reached[(1, 0)], reached[(0, 1)], reached[(1, 1)]))
    assert reached[(0, 1)] > reached[(1, 0)]
    assert max(reached[(0, 1)], reached[(1, 1)]) > reached[(1, 0)]
