"""Episode boundaries without a GPU (include/rem2d_episode.h): the episode model has teeth on the oracle alone, the header, the
ctypes binding and the three libraries agree, rem2d_worlds_reset_where refuses bad arguments before anything is dereferenced, and
reset_where() / set_autoreset() raise what they document.

The GPU half (tests/test_episodes_gpu.py) holds the kernel to tests/episode_model.py and to freshly reset worlds; this half makes
sure that the model is no vacuous yardstick: episodes do end, at many different steps, and a creature's second episode repeats its
first."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import episode_model as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_model_has_teeth(oracle):
    """320 open-loop steps of the L-system loop population with when = ("done",): every creature ends an episode, at least 100 of
    the 119 end two, first episodes end at 20 or more distinct steps, and a creature's second episode has the length and the fitness
    of its first (a reset gives back the same b2World).  Nobody comes near the default build's contact slots."""
    r = EM.run(oracle, "lsystem", EM.N_OPEN, ("done",))
    per = [c for bucket in EM.episode_lengths(r) for c in bucket]
    assert len(per) == 119 and sorted(ctx.K for ctx in r["ctxs"]) == [2, 4, 8, 16]
    assert all(len(c) >= 1 for c in per)
    twice = [c for c in per if len(c) >= 2]
    firsts = {c[0][0] for c in per}
    print("ended twice: %d of %d, %d distinct first ends, first %d, last %d" % (len(twice), len(per), len(firsts), min(firsts), max(firsts)))
    assert len(twice) >= 100 and len(firsts) >= 20
    for c in twice:
        assert c[1][1] == c[0][1] and c[1][2] == c[0][2], c
        assert c[0][1] == c[0][0] and c[1][0] == 2 * c[0][0]          # the length IS the end step; the second ends at twice that
    assert sum(int(k.sum()) for k in r["count"]) == sum(len(c) for c in per)
    assert not any(o.any() for o in r["over"])
    # the harvest's reward / done are the terminal step's: -100 and True wherever an episode ended
    for t, ended in enumerate(r["ended"]):
        for k, e in enumerate(ended):
            assert np.array_equal(r["done"][t][k], e) and (r["reward"][t][k][e] == -100.0).all()


def test_time_limit_episodes_have_that_length(oracle):
    """when = ("steps",), max_steps 60, 130 steps: everyone ends exactly twice, every episode is 60 steps long, and the model stands
    10 steps into a third"""
    r = EM.run(oracle, "lsystem", EM.N_TIMED, ("steps",), EM.TIMED_STEPS)
    for bucket in EM.episode_lengths(r):
        for c in bucket:
            assert [(end, steps) for end, steps, _ in c] == [(60, 60), (120, 60)], c
    assert all((loop.env["steps"] == 10).all() for loop in r["model"].loops)
    assert not any(o.any() for o in r["over"])


def test_selection_rule():
    env = dict(done=np.array([0, 1, 0, 0, 1]), frozen=np.array([0, 0, 1, 0, 1]), steps=np.array([5, 5, 5, 9, 1]))
    sel = lambda *a, **k: EM.selected(env, *a, **k).astype(int).tolist()
    assert sel(("done",), 0) == [0, 1, 0, 0, 1] and sel(("frozen",), 0) == [0, 0, 1, 0, 1] and sel(("steps",), 9) == [0, 0, 0, 1, 0]
    assert sel(("done", "steps"), 5) == [1, 1, 1, 1, 1] and sel(("done", "frozen"), 0) == [0, 1, 1, 0, 1]
    assert sel((), 0, mask=[1, 0, 0, 1, 0]) == [1, 0, 0, 1, 0] and sel(("done",), 0, mask=[1, 1, 0, 0, 0]) == [0, 1, 0, 0, 0]
    with pytest.raises(AssertionError):
        sel((), 0)


def test_header_binding_and_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    with open(os.path.join(ROOT, "include", "rem2d_episode.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*int\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert set(declared) == {"rem2d_episode_abi_version", "rem2d_worlds_reset_where"}
    assert int(re.search(r"#define REM2D_EPISODE_ABI_VERSION (\d+)", text).group(1)) == _lib.EPISODE_ABI_VERSION == 1
    for name, key in (("REM2D_WHEN_DONE", "done"), ("REM2D_WHEN_FROZEN", "frozen"), ("REM2D_WHEN_STEPS", "steps")):
        assert int(re.search(r"#define %s\s+(\d+)" % name, text).group(1)) == _lib.WHEN[key], name
    assert sorted(_lib.WHEN.values()) == [1, 2, 4]
    # the struct: the header's members in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} rem2d_episode_out;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*\w+\s*\*\s*(\w+);", body, flags=re.M)
    assert members == [n for n, _ in _lib.EpisodeOut._fields_] == ["reward", "done", "ended", "fitness", "steps", "episodes"]
    assert C.sizeof(_lib.EpisodeOut) == 6 * 8 and C.sizeof(_lib.Morph) == 20 * 8
    assert "oracle/rem2d_cpu.c" in text and "no counterpart" in " ".join(text.split())      # the header says the twin has none
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in declared:
            assert (" T " + name) in syms, (path, name)
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        assert L.rem2d_episode_abi_version() == _lib.EPISODE_ABI_VERSION and L.rem2d_abi_version() == 11
    # the pinned headers know nothing of it, and rem2d.h is still ABI 11
    for header in ("rem2d.h", "rem2d_control.h", "rem2d_sense.h", "rem2d_policy.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            other = f.read()
        for name in declared + ["REM2D_WHEN_", "REM2D_EPISODE_", "rem2d_episode"]:
            assert name not in other, (header, name)
    with open(os.path.join(ROOT, "include", "rem2d.h")) as f:
        main = f.read()
    assert "#define REM2D_ABI_VERSION 11 " in main
    # ... and the CPU twin has no counterpart
    for name in os.listdir(os.path.join(ROOT, "oracle")):
        if name.endswith((".c", ".h", ".py")):
            with open(os.path.join(ROOT, "oracle", name)) as f:
                assert "reset_where" not in f.read(), name


def _morphs(n):
    from gym_rem2d_amd import _lib
    arr = (_lib.Morph * n)()
    for m in arr:
        for k in _lib.MORPH_FIELDS:
            setattr(m, k, 256)                   # "device pointers" that are never dereferenced: the checks come first
    return arr


def test_bad_arguments_are_refused_before_anything_is_dereferenced():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        err = L.rem2d_last_error
        call = L.rem2d_worlds_reset_where
        fake = (C.c_void_p * 2)(C.c_void_p(8), C.c_void_p(8))    # "worlds" that are never dereferenced
        two = (C.c_void_p * 2)(C.c_void_p(8), None)
        mask = C.c_void_p(256)
        out = _lib.EpisodeOut()
        good = _morphs(2)
        for args, msg in (((None, good, 1, mask, 1, 0, out, 4, None), b"no worlds"),
                          ((fake, good, 0, mask, 1, 0, out, 4, None), b"no worlds"),
                          ((fake, good, -3, mask, 1, 0, out, 4, None), b"no worlds"),
                          ((fake, None, 1, mask, 1, 0, out, 4, None), b"NULL morphologies"),
                          ((fake, good, 1, mask, 8, 0, out, 4, None), b"unknown bits"),
                          ((fake, good, 1, mask, 0x80000001, 0, out, 4, None), b"unknown bits"),
                          ((fake, good, 1, mask, 4, 0, out, 4, None), b"max_steps"),
                          ((fake, good, 1, mask, 5, -60, out, 4, None), b"max_steps"),
                          ((fake, good, 1, None, 0, 0, out, 4, None), b"no mask and no condition"),
                          ((fake, good, 1, None, 0, 60, None, 4, None), b"no mask and no condition"),
                          ((fake, good, 1, mask, 1, 0, out, -1, None), b"negative row count"),
                          ((two, good, 2, mask, 1, 0, out, 4, None), b"world 1 is NULL")):      # before world 0 is looked at
            assert call(*[C.byref(a) if isinstance(a, _lib.EpisodeOut) else a for a in args]) == -1, msg
            assert msg in err() and err().startswith(b"reset_where: "), (msg, err())
        for k in _lib.MORPH_FIELDS:                                   # a NULL member inside the second morphology
            bad = _morphs(2)
            setattr(bad[1], k, None)
            assert call(fake, bad, 2, mask, 1, 0, C.byref(out), 4, None) == -1 and b"morphology 1 has NULL arrays" in err(), k
        assert L.rem2d_abi_version() == 11


class _StubWorld:
    """as far as reset_where's checks look at a world"""
    h = 1

    def __init__(self, device, morph=True):
        self.device, self._morph_dev = device, ({} if morph else None)


def test_python_errors():
    """reset_where / set_autoreset / episodes raise before anything touches a device"""
    import torch
    from gym_rem2d_amd.env import BatchedModular2D, Episodes, when_bits
    env = BatchedModular2D()
    with pytest.raises(ValueError, match="reset first"):
        env.reset_where(when=("done",))
    with pytest.raises(ValueError, match="reset first"):
        env.episodes
    cpu = torch.device("cpu")
    env.worlds, env.n_envs, env._inactive, env._compacted = [(_StubWorld(cpu), None)], 4, set(), False
    ok = torch.ones(4, dtype=torch.bool)
    with pytest.raises(ValueError, match="unknown condition 'dead'"):
        env.reset_where(ok, when=("done", "dead"))
    with pytest.raises(ValueError, match="max_steps > 0"):
        env.reset_where(ok, when=("steps",))
    with pytest.raises(ValueError, match="max_steps > 0"):
        env.reset_where(ok, when=("steps",), max_steps=0)
    with pytest.raises(ValueError, match="neither a mask nor a condition"):
        env.reset_where()
    with pytest.raises(ValueError, match="neither a mask nor a condition"):
        env.reset_where(None, when=(), max_steps=60)
    for bad in (torch.ones(4, dtype=torch.int32), torch.ones(4, dtype=torch.float32), np.ones(4, bool), [True] * 4):
        with pytest.raises(ValueError, match="torch.bool or torch.uint8"):
            env.reset_where(bad)
    for bad in (torch.ones(3, dtype=torch.bool), torch.ones(5, dtype=torch.uint8), torch.ones((4, 1), dtype=torch.bool),
                torch.ones(8, dtype=torch.bool)[::2]):
        with pytest.raises(ValueError, match=r"one entry per creature \[4\]"):
            env.reset_where(bad)
    env.worlds = [(_StubWorld(torch.device("cuda:0")), None)]          # the env's device is another than the mask's
    with pytest.raises(ValueError, match="mask must be on cuda:0, not cpu"):
        env.reset_where(ok)
    # a world without a device morphology: one that compact() made
    env.worlds = [(_StubWorld(cpu, morph=False), None)]
    with pytest.raises(ValueError, match=r"compact\(\)"):
        env.reset_where(ok)
    env.worlds, env._compacted = [(_StubWorld(cpu), None)], True
    with pytest.raises(ValueError, match=r"compact\(\)"):
        env.reset_where(when="done")
    # set_autoreset
    assert env._autoreset is None
    env.set_autoreset()
    assert env._autoreset == (("done", "steps"), 4800)
    env.set_autoreset(when="frozen", max_steps=None)
    assert env._autoreset == (("frozen",), 0)
    env.set_autoreset(None)
    assert env._autoreset is None
    for kw in (dict(when=()), dict(when=("done", "never")), dict(when=("steps",), max_steps=0), dict(when=("steps",), max_steps=None),
               dict(max_steps=-5)):
        with pytest.raises(ValueError):
            env.set_autoreset(**kw)
    assert env._autoreset is None
    assert when_bits(("done", "frozen", "steps")) == 7 and when_bits("steps") == 4 and when_bits(()) == 0 and when_bits(None) == 0
    # the record: population-order buffers of these types (on the host here)
    ep = Episodes(4, cpu)
    assert [getattr(ep, f).dtype for f in Episodes.FIELDS] == [torch.float32, torch.bool, torch.bool, torch.float64, torch.int32, torch.int32]
    assert all(getattr(ep, f).shape == (4,) and not getattr(ep, f).any() for f in Episodes.FIELDS)
    d = ep.descriptor()
    assert d.reward == ep.reward.data_ptr() and d.episodes == ep.count.data_ptr() and d.ended == ep.ended.data_ptr()
    env.worlds = []
