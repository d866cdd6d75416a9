"""Streaming evaluation without a GPU (include/rem2d_stream.h): the stream model has teeth on the oracle alone, the tile table of
the flexible tile shapes does not depend on the creatures (and that of a static shape does: why those are refused), the header, the
ctypes binding and the three libraries agree, rem2d_worlds_refill refuses bad arguments before anything is dereferenced, and
reset_stream() / refill() / compact() / run_stream() raise what they document.

The GPU half (tests/test_stream_gpu.py) holds the kernel to tests/stream_model.py, to the same population uploaded as a whole and to
freshly reset worlds."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import control_model as M
import stream_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_model_has_teeth(oracle):
    """The 119 creatures of the L-system loop population, 125 steps in chunks of 25: at least 40 end by freezing and at least 40 by
    the step limit (so both conditions and both kinds of harvest are exercised), the frozen ones at more than one boundary, and
    nobody comes near the default build's 24 / 6 contact slots."""
    r = SM.run(oracle, "lsystem")
    assert [(c.K, c.N) for c in r["ctxs"]] == [(2, 16), (4, 40), (8, 23), (16, 40)]
    how = np.concatenate(r["how"])
    steps = np.concatenate(r["steps"])
    frozen, limit = int((how == "frozen").sum()), int((how == "steps").sum())
    print("ended by freezing: %d, by the step limit: %d; frozen at boundaries %s" % (frozen, limit, sorted(set(steps[how == "frozen"].tolist()))))
    assert frozen + limit == 119 and frozen >= 40 and limit >= 40
    assert (steps[how == "steps"] == SM.MAX_STEPS).all() and (steps % SM.CHUNK == 0).all() and (steps > 0).all()
    assert len(set(steps[how == "frozen"].tolist())) >= 2
    assert not any(o.any() for o in r["over"])
    fit = np.concatenate(r["fitness"])
    assert np.isfinite(fit).all() and len(set(fit.tolist())) >= 30                   # a mis-copied creature would show


# ------------------------------------------------------------------------------------------------ the tile table and the morphology
def _raw(n, K, parent_of, jround_of):
    parent = np.full((n, K), -1, np.int32)
    jround = np.zeros((n, K), np.int32)
    for k in range(1, K):
        parent[:, k] = parent_of(k)
        jround[:, k] = jround_of(k)
    return parent.reshape(-1), jround.reshape(-1)


def _morphologies(n, K):
    """(parent, jround) arrays [n * K] of unrelated populations of one shape: two L-system draws, full chains, full stars (every
    joint on the root, one schedule phase after the other), and full chains whose joints all sit in ONE phase"""
    from gym_rem2d_amd import synthetic
    from gym_rem2d_amd.compiler import Morphology
    out = []
    for seed0 in (0, 5000):
        m = Morphology.from_specs(synthetic.lsystem_specs(range(seed0, seed0 + n), max_modules=K - 1), K)
        assert m.n_envs == n and m.lanes == K
        out.append((m.arrays["parent"], m.arrays["jround"]))
    if K <= 16:
        m = synthetic.chain_population(n, K, "left", lanes=K)
        out.append((m.arrays["parent"], m.arrays["jround"]))
    out.append(_raw(n, K, lambda k: k - 1, lambda k: (2 << 16) | ((k - 1) % 2)))          # a chain's matching, at any K
    P = min(4, K - 1)
    out.append(_raw(n, K, lambda k: 0, lambda k: (P << 16) | ((k - 1) % P)))
    out.append(_raw(n, K, lambda k: k - 1, lambda k: (1 << 16)))
    return out


@pytest.mark.parametrize("shape", [1, 2, 3])
def test_flexible_tile_tables_do_not_depend_on_the_morphology(shape):
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    passes = {1: 2, 2: 3, 3: 1}[shape]
    for wide in (False, True):
        for K in (2, 4, 8, 16, 32, 64):
            per = 64 // K
            for n in sorted({3 * per + 1 if K < 64 else 5, 2 * per, 7 * per + max(1, per // 2)}):
                n_padded = -(-n // per) * per
                tables = [_lib.plan_tiles(p, j, n, K, n_padded, tile_shape=shape, wide=wide) for p, j in _morphologies(n, K)]
                cap = min(32, passes * 64 // K)                                # creature cap of a tile: the only thing that closes one
                want = list(range(0, n_padded, cap)) + [n_padded]
                for t in tables:
                    assert t.tolist() == want, (shape, wide, K, n, t.tolist(), want)


def test_a_static_tile_table_depends_on_the_morphology():
    """shape 4, 8 lanes: chains with their joints in two alternating phases fill 128-lane tiles (16 creatures, 56 joints a phase); the
    same chains with every joint in ONE phase close a tile after 9 creatures (63 joints).  This pair is why rem2d_worlds_refill
    refuses worlds on the static shapes 0 and 4."""
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    n, K = 40, 8
    two = _raw(n, K, lambda k: k - 1, lambda k: (2 << 16) | ((k - 1) % 2))
    one = _raw(n, K, lambda k: k - 1, lambda k: (1 << 16))
    a, b = (_lib.plan_tiles(p, j, n, K, n, tile_shape=4) for p, j in (two, one))
    assert a.tolist() == [0, 16, 32, 40] and b.tolist() == [0, 9, 18, 27, 36, 40]
    a3, b3 = (_lib.plan_tiles(p, j, n, K, n, tile_shape=3) for p, j in (two, one))
    assert a3.tolist() == b3.tolist() == [0, 8, 16, 24, 32, 40]


# ------------------------------------------------------------------------------------------------------------ header, binding, builds
def test_header_binding_and_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    with open(os.path.join(ROOT, "include", "rem2d_stream.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*int\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert set(declared) == {"rem2d_stream_abi_version", "rem2d_worlds_refill"}
    assert int(re.search(r"#define REM2D_STREAM_ABI_VERSION (\d+)", text).group(1)) == _lib.STREAM_ABI_VERSION == 1
    # the structs: the header's members in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} rem2d_feed;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = re.findall(r"(\w+)\s*[,;]", body)
    assert members == [n for n, _ in _lib.Feed._fields_] == ["M", "id", "count", "lanes", "cursor"], members
    assert C.sizeof(_lib.Feed) == 20 * 8 + 8 + 4 + 4 + 8 and _lib.Feed.cursor.offset == 176 and _lib.Feed.lanes.offset == 172
    body = re.search(r"typedef struct \{([^}]*)\} rem2d_stream_out;", text, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", body) == [n for n, _ in _lib.StreamOut._fields_] == ["fitness", "steps", "err", "finished"]
    assert C.sizeof(_lib.StreamOut) == 4 * 8
    assert "oracle/rem2d_cpu.c" in text and "no counterpart" in " ".join(text.split())      # the header says the twin has none
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in declared:
            assert (" T " + name) in syms, (path, name)
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        assert L.rem2d_stream_abi_version() == _lib.STREAM_ABI_VERSION and L.rem2d_abi_version() == 11
        assert L.rem2d_episode_abi_version() == _lib.EPISODE_ABI_VERSION == 1
    # the other headers know nothing of it, and rem2d.h is still ABI 11
    for header in ("rem2d.h", "rem2d_control.h", "rem2d_sense.h", "rem2d_policy.h", "rem2d_episode.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            other = f.read()
        for name in declared + ["REM2D_STREAM_", "rem2d_feed", "rem2d_stream"]:
            assert name not in other, (header, name)
    with open(os.path.join(ROOT, "include", "rem2d.h")) as f:
        assert "#define REM2D_ABI_VERSION 11 " in f.read()
    # ... and the CPU twin has no counterpart
    for name in os.listdir(os.path.join(ROOT, "oracle")):
        if name.endswith((".c", ".h", ".py")):
            with open(os.path.join(ROOT, "oracle", name)) as f:
                assert "refill" not in f.read(), name
    # build()'s export list names the two symbols
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        entry = f.read()
    assert all('"%s"' % name in entry for name in declared)


# ---------------------------------------------------------------------------------------------------------------- bad arguments
def _morphs(n):
    from gym_rem2d_amd import _lib
    arr = (_lib.Morph * n)()
    for m in arr:
        for k in _lib.MORPH_FIELDS:
            setattr(m, k, 256)                   # "device pointers" that are never dereferenced: the checks come first
    return arr


def _feeds(n, count=3, lanes=4, cursor=256, full=True):
    from gym_rem2d_amd import _lib
    arr = (_lib.Feed * n)()
    for f in arr:
        f.count, f.lanes, f.cursor = count, lanes, cursor
        if full:
            f.id = 256
            for k in _lib.MORPH_FIELDS:
                setattr(f.M, k, 256)
    return arr


def _stub_worlds(lanes, device=(0, 0)):
    """World handles as far as the checks read them before the state checks: rem2d_world_cfg (n_envs, lanes, flags, device) leads the
    handle; everything behind it is zero -- tile shape 0, a static one, and never reset."""
    bufs = []
    for K, dev in zip(lanes, device):
        b = (C.c_int32 * 16384)()
        b[0], b[1], b[2], b[3] = 5, K, 1, dev
        bufs.append(b)
    return (C.c_void_p * len(bufs))(*[C.addressof(b) for b in bufs]), bufs


def test_bad_arguments_are_refused_before_anything_is_dereferenced():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    E_INVALID, E_STATE = -1, -3
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        err = L.rem2d_last_error
        call = L.rem2d_worlds_refill
        fake = (C.c_void_p * 2)(C.c_void_p(8), C.c_void_p(8))    # "worlds" that are never dereferenced
        two = (C.c_void_p * 2)(C.c_void_p(8), None)
        occ = C.c_void_p(256)
        out = _lib.StreamOut()
        good, feeds = _morphs(2), _feeds(2)
        for args, msg in (((None, good, 1, feeds, occ, 2, 0, out, 9, 4, None), b"no worlds"),
                          ((fake, good, 0, feeds, occ, 2, 0, out, 9, 4, None), b"no worlds"),
                          ((fake, good, -3, feeds, occ, 2, 0, out, 9, 4, None), b"no worlds"),
                          ((fake, None, 1, feeds, occ, 2, 0, out, 9, 4, None), b"NULL morphologies"),
                          ((fake, good, 1, None, occ, 2, 0, out, 9, 4, None), b"NULL feeds"),
                          ((fake, good, 1, feeds, None, 2, 0, out, 9, 4, None), b"NULL occupant"),
                          ((fake, good, 1, feeds, occ, 8, 0, out, 9, 4, None), b"unknown bits"),
                          ((fake, good, 1, feeds, occ, 0x80000002, 0, out, 9, 4, None), b"unknown bits"),
                          ((fake, good, 1, feeds, occ, 0, 0, out, 9, 4, None), b"no condition"),
                          ((fake, good, 1, feeds, occ, 0, 125, None, 9, 4, None), b"no condition"),
                          ((fake, good, 1, feeds, occ, 4, 0, out, 9, 4, None), b"max_steps"),
                          ((fake, good, 1, feeds, occ, 6, -125, out, 9, 4, None), b"max_steps"),
                          ((fake, good, 1, feeds, occ, 2, 0, out, 9, -1, None), b"negative row count"),
                          ((fake, good, 1, feeds, occ, 2, 0, out, -9, 4, None), b"negative id count"),
                          ((two, good, 2, feeds, occ, 2, 0, out, 9, 4, None), b"world 1 is NULL")):      # before world 0 is looked at
            assert call(*[C.byref(a) if isinstance(a, _lib.StreamOut) else a for a in args]) == E_INVALID, msg
            assert msg in err() and err().startswith(b"refill: "), (msg, err())
        for k in _lib.MORPH_FIELDS:                                   # a NULL member inside the second morphology ...
            bad = _morphs(2)
            setattr(bad[1], k, None)
            assert call(fake, bad, 2, feeds, occ, 2, 0, C.byref(out), 9, 4, None) == E_INVALID and b"morphology 1 has NULL arrays" in err(), k
            bad = _feeds(2)                                           # ... and inside the second feed, which has pending creatures
            setattr(bad[1].M, k, None)
            assert call(fake, good, 2, bad, occ, 2, 0, C.byref(out), 9, 4, None) == E_INVALID and b"feed 1 has pending creatures and NULL arrays" in err(), k
        bad = _feeds(2)
        bad[1].id = None
        assert call(fake, good, 2, bad, occ, 2, 0, C.byref(out), 9, 4, None) == E_INVALID and b"feed 1 has pending" in err()
        bad = _feeds(2)
        bad[0].count = -1
        assert call(fake, good, 2, bad, occ, 2, 0, C.byref(out), 9, 4, None) == E_INVALID and b"feed 0 has a negative count" in err()
        bad = _feeds(2)
        bad[1].cursor = None
        assert call(fake, good, 2, bad, occ, 2, 0, C.byref(out), 9, 4, None) == E_INVALID and b"feed 1 has no cursor" in err()
        # the worlds, on stubs: lanes, devices, the feed's lane count -- and the static tile shape, ahead of "never reset"
        empty = _feeds(2, count=0, full=False)                        # count == 0: NULL arrays are fine
        stubs, keep = _stub_worlds((4, 128))
        assert call(stubs, good, 2, empty, occ, 2, 0, C.byref(out), 9, 4, None) == E_INVALID and b"more than 64 lanes" in err()
        stubs, keep = _stub_worlds((4, 4), device=(0, 1))
        assert call(stubs, good, 2, empty, occ, 2, 0, C.byref(out), 9, 4, None) == E_INVALID and b"share a device" in err()
        stubs, keep = _stub_worlds((4, 8))
        assert call(stubs, good, 2, empty, occ, 2, 0, C.byref(out), 9, 4, None) == E_INVALID
        assert b"feed 1 holds creatures of 4 lanes, its world creatures of 8" in err()
        stubs, keep = _stub_worlds((4, 4))
        assert call(stubs, good, 2, empty, occ, 2, 0, C.byref(out), 9, 4, None) == E_STATE
        assert b"static tile shape 0" in err() and b"planned from the joints" in err(), err()
        assert call(stubs, good, 2, feeds, occ, 6, 125, None, 0, 0, None) == E_STATE and b"planned from the joints" in err()
        assert L.rem2d_abi_version() == 11


# ---------------------------------------------------------------------------------------------------------------- Python errors
class _StubWorld:
    h = 1

    def __init__(self, device):
        self.device, self._morph_dev = device, {}


def test_slot_rule():
    from gym_rem2d_amd.env import stream_slots
    counts, lanes = [16, 40, 23, 40], [2, 4, 8, 16]
    got = stream_slots(counts, lanes, 40)
    # proportional shares 5.38 / 13.45 / 7.73 / 13.45: the whole parts (38), then the largest remainders (ties to the earlier bucket)
    assert got == [5, 14, 8, 13] and sum(got) == 40
    assert stream_slots(counts, lanes, 4) == [1, 1, 1, 1]
    assert stream_slots(counts, lanes, 119) == counts == stream_slots(counts, lanes, 5000)
    # a wavefront of slots per bucket (32 / 16 / 8 / 4, or all it has) where the window covers them
    got = stream_slots(counts, lanes, 60)
    assert sum(got) == 60 and all(g >= min(c, 64 // K) for g, c, K in zip(got, counts, lanes)) and got[0] == 16
    got = stream_slots([100000, 50, 100000], [2, 16, 4], 1000)
    assert sum(got) == 1000 and got[1] >= 4 and abs(got[0] - got[2]) <= 1
    for slots in (0, 1, 3, -5):
        with pytest.raises(ValueError, match="below the number of lane buckets"):
            stream_slots(counts, lanes, slots)


def test_python_errors(monkeypatch):
    """refill / stream / compact / reset_stream / run_stream raise before anything touches a device"""
    import torch
    from gym_rem2d_amd import evaluate
    from gym_rem2d_amd.env import BatchedModular2D
    terrain, morphs = M.loop_population("lsystem")
    batches, at = [], 0
    for m in morphs:
        batches.append((m, np.arange(at, at + m.n_envs)))
        at += m.n_envs
    env = BatchedModular2D(flags=evaluate.EVAL_FLAGS)
    with pytest.raises(ValueError, match="reset_stream first"):
        env.refill()
    with pytest.raises(ValueError, match="reset_stream first"):
        env.stream
    cpu = torch.device("cpu")
    env.worlds, env.n_envs, env._inactive, env._compacted = [(_StubWorld(cpu), None)], 4, set(), False
    with pytest.raises(ValueError, match="reset_stream first"):      # a population in place, uploaded as a whole
        env.refill(max_steps=125)
    # slots below the number of buckets; batches that are not the whole population
    for slots in (0, 3):
        with pytest.raises(ValueError, match="below the number of lane buckets"):
            env.reset_stream(batches, 119, slots)
    with pytest.raises(ValueError, match="every creature of the population"):
        env.reset_stream(batches, 120, 40)
    with pytest.raises(ValueError, match="every creature of the population"):
        env.reset_stream(batches[:3], 119, 40)
    # a plan on a static tile shape, through the override
    monkeypatch.setenv("REM2D_TILE_SHAPE", "4")
    with pytest.raises(ValueError, match="static tile shape 4"):
        env.reset_stream(batches, 119, 40)
    monkeypatch.delenv("REM2D_TILE_SHAPE")
    env.tile_shape = 0
    with pytest.raises(ValueError, match="static tile shape 0"):
        env.reset_stream(batches, 119, 40)
    env.tile_shape = None
    assert env.worlds[0][0].h == 1                                   # nothing above got as far as the upload
    # a streamed env: compact() raises, refill() checks its conditions
    env._stream_rec = object()
    with pytest.raises(ValueError, match="compact: this env streams"):
        env.compact()
    with pytest.raises(ValueError, match="unknown condition 'dead'"):
        env.refill(when=("frozen", "dead"))
    with pytest.raises(ValueError, match="at least one condition"):
        env.refill(when=())
    with pytest.raises(ValueError, match="max_steps > 0"):
        env.refill()
    with pytest.raises(ValueError, match="max_steps > 0"):
        env.refill(when=("steps",), max_steps=0)
    env._stream_rec = None
    # run_stream
    with pytest.raises(ValueError, match="multiple of chunk"):
        evaluate.run_stream(env, batches, 119, 40, max_steps=125, chunk=100)
    with pytest.raises(ValueError, match="multiple of chunk"):
        evaluate.run_stream(env, batches, 119, 40, max_steps=100, chunk=0)
    with pytest.raises(ValueError, match="on_error"):
        evaluate.run_stream(env, batches, 119, 40, on_error="shrug")
    plain = BatchedModular2D()
    with pytest.raises(ValueError, match="REM2D_FLAG_SKIP_FROZEN"):
        evaluate.run_stream(plain, batches, 119, 40, max_steps=125, chunk=25)
    with pytest.raises(ValueError, match="below the number of lane buckets"):
        evaluate.run_stream(env, batches, 119, 2, max_steps=125, chunk=25)
    env.worlds = []
