"""The creature order without a GPU (include/rem2d_order.h): tests/order_model.py is held to numpy's stable argsort and to the pins
the suite already has, the sizes of tests/test_order_gpu.py land on the thread counts it claims, the header, the ctypes binding
and the three libraries agree, and the two calls refuse bad arguments before anything is dereferenced.

The GPU half (tests/test_order_gpu.py) holds rem2d_rebalance_kernel, the host paths and the cadence of the `rebalance` launch option
to the model."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import order_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the model
def _inputs(pos_iters):
    """(name, positers): random and adversarial"""
    rng = np.random.default_rng(pos_iters)
    values = np.array([0, 1, 2, 3, 4, pos_iters - 1, pos_iters, pos_iters + 1, 8191], np.int32)
    for n in (1, 2, 3, 63, 64, 65, 257, 1000, 4099):
        e = np.arange(n)
        yield "random %d" % n, values[rng.integers(0, len(values), n)]
        yield "any int %d" % n, rng.integers(-5, 70, n).astype(np.int32)
        for v in (0, 2, 3, pos_iters - 1, pos_iters, pos_iters + 1):
            yield "all %d x %d" % (v, n), np.full(n, v, np.int32)
        yield "alternating %d" % n, np.where(e % 2 == 0, pos_iters, 0).astype(np.int32)
        yield "alternating 3 / 2 %d" % n, np.where(e % 2 == 0, 2, 3).astype(np.int32)
        thirds = np.minimum(e * 3 // n, 2)
        yield "ascending %d" % n, np.array([pos_iters, 3, 0], np.int32)[thirds]
        yield "descending %d" % n, np.array([0, 3, pos_iters], np.int32)[thirds]
        for i in {0, n // 2, n - 1}:
            p = np.zeros(n, np.int32)
            p[i] = pos_iters
            yield "one heavy at %d of %d" % (i, n), p


@pytest.mark.parametrize("pos_iters", [1, 2, 3, 4, 60])
def test_device_order_is_the_stable_sort_by_class(pos_iters):
    seen = set()
    for name, p in _inputs(pos_iters):
        n = len(p)
        cls = M.cost_class(p, pos_iters)
        want_cls = [0 if v >= pos_iters else (1 if v >= 3 else 2) for v in p.tolist()]      # the sentence, creature by creature
        assert cls.tolist() == want_cls, name
        seen |= set(want_cls)
        for n_padded in (n, n + 1, -(-n // 32) * 32):
            got = M.device_order(p, pos_iters, n_padded)
            assert got.dtype == np.int32 and got.shape == (2, n_padded), name
            assert np.array_equal(got[0, :n], np.argsort(cls, kind="stable")), name
            assert np.array_equal(got[0, n:], np.arange(n, n_padded)), name                # padding is the identity
            assert np.array_equal(got[0], got[1]), name
            assert np.array_equal(np.sort(got[0]), np.arange(n_padded)), name              # always a permutation
            assert M.is_valid(got, n, n_padded), name
        host = M.host_order(p, pos_iters)
        assert np.array_equal(host, np.argsort(~(p >= pos_iters), kind="stable")), name      # what BatchedModular2D.rebalance() sorts
        assert np.array_equal(np.sort(host), np.arange(n)), name
        two = M.device_order(p, pos_iters, n, classes=2)
        assert np.array_equal(two[0], host), name
    # pos_iters <= 3 leaves no middle class: three or more iterations are all of them
    assert seen == ({0, 2} if pos_iters <= 3 else {0, 1, 2})


def test_is_valid_refuses_what_it_must():
    n, n_padded = 5, 8
    good = M.identity(n_padded)
    good[:, :n] = [4, 2, 0, 1, 3]
    assert M.is_valid(good, n, n_padded)
    for change in ((0, 1, 4), (1, 0, 0), (0, 6, 5), (0, 0, 5), (0, 0, -1)):             # (half, slot, value)
        bad = good.copy()
        bad[change[0], change[1]] = change[2]
        assert not M.is_valid(bad, n, n_padded), change
    dup = good.copy()
    dup[:, 1] = 4                                                                       # equal halves, creature 4 twice, 2 never
    assert not M.is_valid(dup, n, n_padded)
    swapped = good.copy()
    swapped[:, [4, 5]] = swapped[:, [5, 4]]                                             # a padding slot among the creatures
    assert not M.is_valid(swapped, n, n_padded)
    assert not M.is_valid(good[:, :7], n, n_padded) and not M.is_valid(good[0], n, n_padded)


def test_threads_for_at_every_edge():
    want = {1: 64, 64: 64, 65: 64, 4096: 64, 16384: 64, 16385: 128, 32768: 128, 32769: 256, 65536: 256, 65537: 512, 131072: 512,
            131073: 1024, 262144: 1024, 262145: 1024, 10 ** 6: 1024, 5 * 10 ** 6: 1024}
    for n, t in want.items():
        assert M.threads_for(n) == t, n
    # ... and what the rule is for: a thread's chunk stays at <= 256 creatures up to the largest workgroup's 262 144
    for n in list(want) + list(range(1, 300000, 4099)):
        t = M.threads_for(n)
        assert t in (64, 128, 256, 512, 1024)
        if n <= 262144:
            assert M.chunk(n) <= 256, n
            assert t == 64 or (t // 2) * 256 < n, n                                     # no more threads than that takes
        per = M.chunk(n)
        assert per * t >= n > (per - 1) * t
    # the launch code says the same thing (csrc/rem2d.hip launch_rebalance), and the kernel's cap is the model's
    with open(os.path.join(ROOT, "gym_rem2d_amd", "csrc", "rem2d.hip")) as f:
        src = " ".join(f.read().split())
    assert "int threads = WAVE; while (threads < REBALANCE_MAX_THREADS && threads * 256 < w->cfg.n_envs) threads *= 2;" in src
    with open(os.path.join(ROOT, "gym_rem2d_amd", "csrc", "rem2d_pipeline.h")) as f:
        pipe = f.read()
    assert "#define REBALANCE_MAX_THREADS 1024" in pipe and M.MAX_THREADS == 1024 and M.CHUNK == 256 and M.WAVE == 64
    assert re.search(r"#define REBALANCE_CLASSES 3\b", pipe)


def test_sizes_of_the_gpu_test_land_on_their_thread_counts():
    """Every (size, threads) pair of tests/test_order_gpu.py, the issue's table among them: all five thread counts, both sides of
    every threshold, an empty tail thread at 256 / 512 / 1 024 threads, and padding slots in the worlds that are there for them"""
    import test_order_gpu as G
    assert [s[0] for s in G.SIZES] == [1, 2, 63, 64, 65, 16384, 16385, 16511, 32768, 32769, 65536, 65537, 131072, 131073, 150001]
    for n, threads in G.SIZES:
        assert M.threads_for(n) == threads, n
    assert sorted({t for _, t in G.SIZES}) == [64, 128, 256, 512, 1024]
    for edge in (16384, 32768, 65536, 131072):
        assert {edge, edge + 1} <= {s[0] for s in G.SIZES}
    for n, threads in ((32769, 256), (65537, 512), (131073, 1024), (150001, 1024), (1, 64), (63, 64)):
        assert M.chunk(n, threads) * (threads - 1) >= n                                 # the last thread's chunk is empty
    assert M.chunk(16511, 128) * 127 < 16511 < M.chunk(16511, 128) * 128                # ... and here it is one short
    for n, lanes, threads in G.PADDED:
        per = 64 // lanes
        assert M.threads_for(n) == threads > 64 and -(-n // per) * per > n and lanes in (8, 32)
    assert {lanes for _, lanes, _ in G.PADDED} == {8, 32}
    for n, wide in G.OTHER_BUILDS:
        assert wide in (True, "fma")
    assert G.POS_ITERS == (60, 3, 1)
    # the patterns: the issue's list, and the single heavy creature at both ends and at chunk edges of the first and last threads
    for n, threads in G.SIZES:
        names = [name for name, p in G.patterns(n, 60, threads)]
        for must in ("all 0", "all heavy", "alternating", "ascending class", "descending class", "random", "1 % heavy",
                     "heavy at 0", "heavy at %d" % (n - 1)):
            assert must in names, (n, must)
        per = M.chunk(n, threads)
        if n > per:
            assert "heavy at %d" % (per - 1) in names and "heavy at %d" % per in names
        for name, p in G.patterns(n, 60, threads):
            assert p.shape == (n,) and p.dtype == np.int32, name


def test_reorder_points_reproduce_the_pinned_train():
    """tests/test_launch_forms_gpu.py::test_train_is_cut_where_a_reordering_is_due: rebalance_every = 2, calls (1, 3, 7) on the step
    train go in launches 1 | 2 1 | 2 2 2 1 -- seven launches, the count that test pins"""
    import test_launch_forms_gpu as F
    assert F.CALLS == (1, 3, 7)
    segs = M.train_segments(F.CALLS, 2)
    assert segs == [[1], [2, 1], [2, 2, 2, 1]] and sum(len(s) for s in segs) == 1 + 2 + 4
    assert M.train_segments(F.CALLS, 0) == [[1], [3], [7]]
    # a launch re-orders once `every` or more steps have been queued since the last one that did
    assert M.reorder_points(F.CALLS, 2, "train") == [[], [3], [6, 8, 10]]
    assert M.reorder_points(F.CALLS, 2, "step") == [[], [2], [4, 6, 8, 10]]
    # what tests/test_order_gpu.py runs
    assert M.reorder_points((1, 3, 7, 2), 3, "step") == [[], [3], [6, 9], [12]]
    assert M.reorder_points((1, 3, 7, 2), 3, "train") == [[], [], [4, 7, 10], []]
    assert M.reorder_points((3, 3, 3, 3), 3, "step") == [[], [3], [6], [9]]
    assert M.reorder_points((3, 3, 3, 3), 3, "train") == [[], [3], [6], [9]]
    # two short trains drain twice: a call is cut only where it is itself longer than `every`
    assert M.reorder_points((2, 2, 2, 2), 3, "train") == [[], [], [4], []]
    assert M.reorder_points((2, 2, 2, 2), 3, "step") == [[], [3], [], [6]]
    # nothing is re-ordered in front of a world's very first step, whatever has been queued is counted from its creation
    assert M.reorder_points((3,), 3, "step", queued0=3) == [[3]] and M.reorder_points((3,), 3, "step") == [[]]
    assert M.reorder_points((1, 1), 1, "step") == [[], [1]] and M.reorder_points((5,), 0, "step") == [[]]
    with pytest.raises(ValueError):
        M.reorder_points((1,), 1, "graph")


def test_the_model_restates_the_cadence_comments():
    """the sentences of csrc/rem2d.hip the model was written from are still there"""
    with open(os.path.join(ROOT, "gym_rem2d_amd", "csrc", "rem2d.hip")) as f:
        src = " ".join(f.read().split())
    for sentence in ("w->stepsQueued > 0 && w->stepsQueued % every == 0 && (w->S.flags & REM2D_STATE_ORDERED)",
                     "w->stepsQueued > 0 && w->stepsQueued - w->stepsAtOrder >= every && (w->S.flags & REM2D_STATE_ORDERED)",
                     "if (every > 0 && seg > every) seg = every;",
                     "a call is cut only where it is itself longer than N steps"):
        assert sentence in src, sentence


# ------------------------------------------------------------------------------------------------------------ header, binding, builds
EXPORTS = {"rem2d_order_abi_version", "rem2d_world_read_order", "rem2d_world_make_order"}


def test_header_binding_and_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    with open(os.path.join(ROOT, "include", "rem2d_order.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*int\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert set(declared) == EXPORTS and len(declared) == 3
    assert int(re.search(r"#define REM2D_ORDER_ABI_VERSION (\d+)", text).group(1)) == _lib.ORDER_ABI_VERSION == 1
    assert "oracle/rem2d_cpu.c" in text and "no counterpart" in " ".join(text.split())      # the header says the twin has none
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        exported = set(re.findall(r" T (rem2d_\w*order\w*)", syms))
        assert exported == EXPORTS | {"rem2d_world_set_order"}, (path, exported)           # set_order: include/rem2d.h, as before
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        assert L.rem2d_order_abi_version() == _lib.ORDER_ABI_VERSION and L.rem2d_abi_version() == 11
        assert L.rem2d_world_read_order.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p]
        assert L.rem2d_world_make_order.argtypes == [C.c_void_p, C.c_int32, C.c_void_p]
    # the other headers know nothing of it, and rem2d.h is still ABI 11
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header == "rem2d_order.h":
            continue
        with open(os.path.join(ROOT, "include", header)) as f:
            other = f.read()
        for name in sorted(EXPORTS) + ["REM2D_ORDER_"]:
            assert name not in other, (header, name)
    with open(os.path.join(ROOT, "include", "rem2d.h")) as f:
        assert "#define REM2D_ABI_VERSION 11 " in f.read()
    # ... the CPU twin has no counterpart, and its test lists the names among the entry points without one
    for name in os.listdir(os.path.join(ROOT, "oracle")):
        if name.endswith((".c", ".h", ".py")):
            with open(os.path.join(ROOT, "oracle", name)) as f:
                src = f.read()
            assert "read_order" not in src and "make_order" not in src, name
    import test_cpu_twin
    assert {"rem2d_world_read_order", "rem2d_world_make_order"} <= test_cpu_twin.HOST_ONLY
    # build()'s export list and the integration guide name the symbols
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        entry = f.read()
    assert all('"%s"' % name in entry for name in declared)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        guide = f.read()
    assert all(name in guide for name in declared)
    # the wrapper's methods
    from gym_rem2d_amd.world import BatchedWorld
    assert callable(BatchedWorld.order) and callable(BatchedWorld.make_order)


def _stub_world(flags):
    """A world handle as far as the checks read it: rem2d_world_cfg (n_envs, lanes, flags, device) leads the handle"""
    b = (C.c_int32 * 16384)()
    b[0], b[1], b[2], b[3] = 5, 2, flags, 0
    return b


def test_bad_arguments_are_refused_before_anything_is_dereferenced():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    E_INVALID = -1
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        err = L.rem2d_last_error
        fake, out = C.c_void_p(8), C.c_void_p(256)              # a "world" and an "array" that are never dereferenced
        assert L.rem2d_world_read_order(None, out, None) == E_INVALID and b"read_order: world is NULL" in err()
        assert L.rem2d_world_read_order(fake, None, None) == E_INVALID and b"read_order: NULL output" in err()
        assert L.rem2d_world_make_order(None, 60, None) == E_INVALID and b"make_order: world is NULL" in err()
        retile = _stub_world(1 | _lib.FLAG_RETILE)
        assert L.rem2d_world_make_order(C.addressof(retile), 60, None) == E_INVALID and b"REM2D_FLAG_RETILE" in err()
        plain = _stub_world(1)
        for bad in (0, -1, -2 ** 31):
            assert L.rem2d_world_make_order(C.addressof(plain), bad, None) == E_INVALID, bad
            assert b"make_order: pos_iters must be >= 1" in err()
