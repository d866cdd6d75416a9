"""The creature order a world holds, on a real MI355X (pytest -m gpu): BatchedWorld.order() / make_order() (include/rem2d_order.h)
against tests/order_model.py, under ``==``.

a. rem2d_rebalance_kernel alone, launched by the step paths' own launch_rebalance, at every thread count it can take (64, 128, 256,
   512, 1 024) and at the sizes where the count changes: no world here is ever stepped.
b. the host paths: set_order(perm), set_order(None) with the `rebalance` option off and on, BatchedModular2D.rebalance().
c. the cadence of the `rebalance` option in every launch form: after every step call each world's order is the model's order of that
   world's own creatures at the last re-ordering point.  The position iterations the kernel sorts by come from a twin env stepped
   one step at a time with the option off (results do not depend on the order: tests/test_parity_gpu.py holds that).

Every read is first held to: both halves equal, a permutation, identity padding.  A world that fails this is set back to the arena
order, closed and never stepped.
"""
import ctypes as C

import numpy as np
import pytest

import order_model as M

pytestmark = pytest.mark.gpu

POS_ITERS = (60, 3, 1)
# (creatures, threads the launch takes) of the two-lane worlds: the smallest sizes that reach each path, and the last / first size of
# each thread count
SIZES = [(1, 64), (2, 64), (63, 64), (64, 64), (65, 64), (16384, 64),
         (16385, 128), (16511, 128), (32768, 128),
         (32769, 256), (65536, 256),
         (65537, 512), (131072, 512),
         (131073, 1024), (150001, 1024)]
# (creatures, lanes, threads): the padding loop at work in a launch of more than one wavefront
PADDED = [(16389, 8, 128), (16385, 32, 128)]
# the other two builds, where it costs next to nothing: one wavefront and two, with a short last chunk
OTHER_BUILDS = [(65, True), (16511, True), (65, "fma"), (16511, "fma")]


@pytest.fixture(scope="module")
def gpu():
    import replay
    return replay.need_gpu(world=True)


def read_checked(w):
    """order() on the host, after it has passed order_model.is_valid -- or the world set back to the arena order and closed"""
    import torch
    got = w.order()
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    if not M.is_valid(got, w.n_envs, w.n_envs_padded):
        n, npad = w.n_envs, w.n_envs_padded
        w.set_order(None)          # (an order that is no permutation must not reach a step kernel)
        w.close()
        bad = np.nonzero(got[0] != got[1])[0]
        raise AssertionError("order of a %d-creature world (%d slots) is not a permutation with identity padding in two equal "
                             "halves; halves differ at %s, sorted head == arange: %s, padding: %s"
                             % (n, npad, bad[:8].tolist(), bool(np.array_equal(np.sort(got[0, :n]), np.arange(n))),
                                got[0, n:].tolist()[:8]))
    return got


# ------------------------------------------------------------------------------------------------ a. the kernel, without stepping
def patterns(n, pos_iters, threads):
    """(name, positers int32 [n]): the issue's list; `heavy` = pos_iters, the value of class 0"""
    rng = np.random.default_rng(1000 * n + pos_iters)
    e = np.arange(n)
    heavy = pos_iters
    yield "all 0", np.zeros(n, np.int32)
    yield "all heavy", np.full(n, heavy, np.int32)
    yield "alternating", np.where(e % 2 == 0, heavy, 0).astype(np.int32)
    thirds = np.minimum(e * 3 // max(n, 1), 2)
    by_class = np.array([heavy, 3, 0], np.int32)          # a value of class 0, 1 (where pos_iters > 3 leaves one), 2
    yield "ascending class", by_class[thirds]
    yield "descending class", by_class[2 - thirds]
    values = np.array([0, 2, 3, 4, pos_iters - 1, pos_iters, pos_iters + 1], np.int32)
    yield "random", values[rng.integers(0, len(values), n)]
    yield "1 % heavy", np.where(rng.random(n) < 0.01, heavy, 0).astype(np.int32)
    per = M.chunk(n, threads)
    edges = {0, n - 1}
    for k in sorted({1, 2, threads // 2, threads - 1, -(-n // per) - 1}):   # ... and the last thread that has a chunk at all
        edges |= {k * per - 1, k * per}
    for i in sorted(i for i in edges if 0 <= i < n):
        p = np.zeros(n, np.int32)
        p[i] = heavy
        yield "heavy at %d" % i, p


def kernel_world(BatchedWorld, flat_terrain, n, lanes, wide=False):
    from gym_rem2d_amd import synthetic
    w = BatchedWorld(n, lanes, flags=1, wide=wide)
    w.set_terrain(flat_terrain)
    w.reset(synthetic.chain_population(n, 2, "left", lanes=lanes))     # one two-body creature, replicated with array ops
    return w


def check_kernel(BatchedWorld, flat_terrain, n, lanes, threads, wide=False):
    import time
    import torch
    assert M.threads_for(n) == threads
    t0 = time.perf_counter()
    w = kernel_world(BatchedWorld, flat_terrain, n, lanes, wide)
    try:
        npad = w.n_envs_padded
        first = read_checked(w)
        assert np.array_equal(first, M.identity(npad)), "a new world starts in arena order"
        view = w.view("positers")
        assert view.shape == (n,) and view.dtype == torch.int32
        cases = 0
        for pos_iters in POS_ITERS:
            for name, p in patterns(n, pos_iters, threads):
                view.copy_(torch.from_numpy(p))
                w.make_order(pos_iters)
                got = read_checked(w)
                want = M.device_order(p, pos_iters, npad)
                if not np.array_equal(got, want):
                    bad = np.nonzero(got[0] != want[0])[0]
                    raise AssertionError("n %d lanes %d threads %d pos_iters %d pattern %r: %d slots differ, first %d: got %d, want %d"
                                         % (n, lanes, threads, pos_iters, name, len(bad), bad[0], got[0, bad[0]], want[0, bad[0]]))
                cases += 1
        # make_order touched nothing but the order: the world still does not go through it, and its cadence has not moved
        assert w.get_option("rebalance") == 0
        print("n %d lanes %d: %d threads, %d slots, arena %.1f MB, %d patterns, %.2f s"
              % (n, lanes, threads, npad, w.arena.numel() / 1e6, cases, time.perf_counter() - t0))
    finally:
        if getattr(w, "h", None):
            w.set_order(None)
        w.release()


@pytest.mark.parametrize("n,threads", SIZES, ids=["n%d-t%d" % s for s in SIZES])
def test_kernel_order_equals_the_model(gpu, flat_terrain, n, threads):
    check_kernel(gpu, flat_terrain, n, 2, threads)


@pytest.mark.parametrize("n,lanes,threads", PADDED, ids=["n%d-lanes%d-t%d" % s for s in PADDED])
def test_kernel_order_with_padding_slots(gpu, flat_terrain, n, lanes, threads):
    """lanes 8 and 32: n_padded > n_envs, so the padding loop writes in a launch of two wavefronts"""
    from gym_rem2d_amd import _lib
    cfg = _lib.WorldCfg(n, lanes, 1, 0)
    assert _lib.lib().rem2d_padded_envs(C.byref(cfg)) > n
    check_kernel(gpu, flat_terrain, n, lanes, threads)


@pytest.mark.parametrize("n,wide", OTHER_BUILDS, ids=["n%d-%s" % (n, "wide" if w is True else w) for n, w in OTHER_BUILDS])
def test_kernel_order_in_the_other_builds(gpu, flat_terrain, n, wide):
    check_kernel(gpu, flat_terrain, n, 2, M.threads_for(n), wide=wide)


def test_make_order_refuses_what_the_header_says(gpu, flat_terrain):
    from gym_rem2d_amd import _lib
    w = gpu(40, 2, flags=1)
    for bad in (0, -1):
        with pytest.raises(_lib.Rem2dError, match="pos_iters"):
            w.make_order(bad)
    w.close()
    w = gpu(40, 2, flags=1 | _lib.FLAG_RETILE)
    with pytest.raises(_lib.Rem2dError, match="REM2D_FLAG_RETILE"):
        w.make_order(60)
    w.close()


# ---------------------------------------------------------------------------------------------------------------- b. the host paths
@pytest.mark.parametrize("rebalance", [0, 5], ids=["rebalance-off", "rebalance-on"])
def test_set_order_reads_back(gpu, flat_terrain, rebalance):
    """set_order(perm): perm in both halves + identity padding; set_order(None): the identity, with the option off and on"""
    import torch
    n = 70
    w = kernel_world(gpu, flat_terrain, n, 2)
    try:
        npad = w.n_envs_padded
        assert npad == 96
        if rebalance:
            w.set_option("rebalance", rebalance)
        for seed in (0, 1):
            perm = np.random.default_rng(seed).permutation(n).astype(np.int32)
            w.set_order(torch.from_numpy(perm))
            want = M.identity(npad)
            want[:, :n] = perm
            assert np.array_equal(read_checked(w), want)
        w.set_order(None)
        assert np.array_equal(read_checked(w), M.identity(npad))
        w.set_order(None)                                                # (twice: nothing installed any more)
        assert np.array_equal(read_checked(w), M.identity(npad))
    finally:
        w.release()


@pytest.fixture(scope="module")
def specs(gpu):
    from gym_rem2d_amd import synthetic
    return synthetic.lsystem_specs(range(96), mutate_odd=True)   # the population of tests/test_launch_forms_gpu.py


def make_env(specs, options=None, shape=None, every=0, graph=False, step_groups=1):
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D(seed=4, flags=1, options=options)
    env.tile_shape, env.rebalance_every, env.use_graph, env.step_groups = shape, every, graph, step_groups
    env.reset_specs(specs)
    assert len(env.worlds) >= 3
    return env


def test_host_rebalance_installs_the_host_order(gpu, specs):
    """BatchedModular2D.rebalance(pos_iters) after a step call: order_model.host_order of every world's own positers (worlds of
    fewer than two wavefronts' worth of creatures keep the arena order: rebalance() leaves them out) -- on what the steps left, and
    on an injected mix of values so that no world's answer is the identity by accident"""
    import torch
    env = make_env(specs)
    try:
        env.step(5)
        rng = np.random.default_rng(7)
        moved = 0
        for inject in (False, True):
            for pos_iters in (60, 3):
                if inject:
                    for w, _ in env.worlds:
                        vals = np.array([0, 2, 3, pos_iters - 1, pos_iters, pos_iters + 1], np.int32)
                        w.view("positers").copy_(torch.from_numpy(vals[rng.integers(0, len(vals), w.n_envs)]))
                env.rebalance(pos_iters)
                for w, _ in env.worlds:
                    got = read_checked(w)
                    p = w.view("positers").cpu().numpy()
                    want = M.identity(w.n_envs_padded)
                    if w.n_envs >= 2 * (64 // min(64, w.lanes)):
                        want[:, :w.n_envs] = M.host_order(p, pos_iters)
                    assert np.array_equal(got, want), (inject, pos_iters, w.n_envs, w.lanes)
                    moved += int(not np.array_equal(got, M.identity(w.n_envs_padded)))
        assert moved > 0
        for w, _ in env.worlds:
            w.set_order(None)
            assert np.array_equal(read_checked(w), M.identity(w.n_envs_padded))
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------------------ c. the cadence
EVERY = 3
CALLS = (1, 3, 7, 2)
RESET_AFTER = 2              # the reset case: reset() of every world between calls 2 and 3, after 4 queued steps
REPLAY_CALLS = (3, 3, 3, 3)  # every call the same length and phase: the second, third and fourth replay a captured graph
TWIN_STEPS = 13

# (id, launch options, tile shape, launch_info(), cadence form of order_model.reorder_points, graph replay possible)
FORMS = [("tiles", {"fuse_velpost": 0}, None, (3, 0), "step", True),
         ("velpost", {"fuse_velpost": 1}, None, (3, 1), "step", True),
         ("train", {"fuse_velpost": 2}, None, (3, 2), "train", False),
         ("train128", {"fuse_velpost": 2}, 1, (1, 2), "train", False)]
CASES = [(name, graph, groups) for name, _, _, _, _, can_graph in FORMS for graph in ((False, True) if can_graph else (False,))
         for groups in (1, 3)]


def world_shapes(env):
    return [(w.n_envs, w.lanes, idx.cpu().numpy().tolist()) for w, idx in env.worlds]


def reset_worlds(env):
    """rem2d_world_reset of every world, in place: the worlds (and the steps they have queued since their creation) stay"""
    for (w, _), m in zip(env.worlds, env._world_morph):
        w.reset(m)


_twins = {}


def twin(specs, step_groups, reset_at=None):
    """(world shapes, P): P[wi][q] = positers of world wi after q env-steps, the `rebalance` option off, one step per call, the
    library's default launch form; reset_at: the worlds are reset once q == reset_at steps have run, and P restarts: P[wi][q] is
    then the state after q - reset_at steps of the new episode.  Made once per (step_groups, reset_at)."""
    key = (step_groups, reset_at)
    if key not in _twins:
        import torch
        env = make_env(specs, step_groups=step_groups)
        P = [[] for _ in env.worlds]

        def record():
            torch.cuda.synchronize()
            for wi, (w, _) in enumerate(env.worlds):
                assert w.get_option("rebalance") == 0
                P[wi].append(w.view("positers").cpu().numpy().copy())
        if reset_at == 0:
            reset_worlds(env)
        record()
        for q in range(1, TWIN_STEPS + 1):
            env.step(1)
            if q == reset_at:
                reset_worlds(env)
            record()
        _twins[key] = (world_shapes(env), P)
        env.close()
    return _twins[key]


def run_cadence(specs, form_name, graph, step_groups, calls, reset_after=None):
    """One population through `calls`; after every call each world's order against the model at the last re-ordering point"""
    import torch
    _, options, shape, info, form, _ = next(f for f in FORMS if f[0] == form_name)
    reset_at = None if reset_after is None else sum(calls[:reset_after])
    shapes, P = twin(specs, step_groups, reset_at)
    points = M.reorder_points(calls, EVERY, form)
    env = make_env(specs, options=options, shape=shape, every=EVERY, graph=graph, step_groups=step_groups)
    try:
        assert env.launch_info() == info and len(env.groups) == step_groups
        assert world_shapes(env) == shapes, "the twin holds other creatures in its worlds"
        assert max(len(g) for g in env.groups) >= 2, "no merged launch"
        for w, _ in env.worlds:
            assert w.get_option("rebalance") == EVERY
        last, launches = None, 0
        for ci, n in enumerate(calls):
            if ci == reset_after:
                reset_worlds(env)
            env.step(n)
            torch.cuda.synchronize()
            if points[ci]:
                last = points[ci][-1]
                launches += len(points[ci])
            for wi, (w, _) in enumerate(env.worlds):
                got = read_checked(w)
                want = M.identity(w.n_envs_padded) if last is None else M.device_order(P[wi][last], 60, w.n_envs_padded)
                assert np.array_equal(got, want), \
                    "%s graph %s groups %d: after call %d (%d steps), world %d (%d x %d): not the order of re-ordering point %s" \
                    % (form_name, graph, step_groups, ci, n, wi, w.n_envs, w.lanes, last)
            # the steps themselves: the same positers as the twin's (the order never changes a result); at the reset point the twin
            # recorded the freshly reset state, which this env reaches only in front of its next call
            q = sum(calls[:ci + 1])
            for wi, (w, _) in enumerate(env.worlds):
                if q != reset_at:
                    assert np.array_equal(w.view("positers").cpu().numpy(), P[wi][q]), (wi, q)
        assert int(env.errors().max()) == 0
        moved = sum(int(not np.array_equal(M.device_order(P[wi][last], 60, w.n_envs_padded), M.identity(w.n_envs_padded)))
                    for wi, (w, _) in enumerate(env.worlds))
        print("%s graph %s groups %d: re-ordering points %s, %d worlds, %d of them not in arena order at the end"
              % (form_name, graph, step_groups, points, len(env.worlds), moved))
        return moved
    finally:
        env.close()


@pytest.mark.parametrize("form,graph,groups", CASES, ids=["%s-%s-groups%d" % (f, "graph" if g else "plain", k) for f, g, k in CASES])
def test_cadence_in_every_launch_form(gpu, specs, form, graph, groups):
    """rebalance_every = 3, calls (1, 3, 7, 2): per-step forms re-order in front of queued steps 3, 6, 9, 12; the trains in front of
    the launches at 4, 7, 10 (order_model.reorder_points).  Every world of a merged launch against its own creatures."""
    moved = run_cadence(specs, form, graph, groups, CALLS)
    assert moved > 0, "every world's order is the identity: the case cannot tell a re-ordering from none"


@pytest.mark.parametrize("form", ["velpost", "train"])
def test_cadence_counts_from_creation_across_a_reset(gpu, specs, form):
    """rem2d_world_reset between calls 2 and 3 (4 steps queued): the cadence goes on counting -- per-step forms re-order in front
    of queued steps 6, 9, 12 = after 2, 5, 8 steps of the new episode; the train at 4 (the freshly reset state), 7, 10"""
    run_cadence(specs, form, False, 1, CALLS, reset_after=RESET_AFTER)


@pytest.mark.parametrize("form", ["tiles", "velpost"])
def test_graph_replay_keeps_the_cadence(gpu, specs, form):
    """Four calls of 3 steps at rebalance_every = 3: all start at phase 0 of the cadence, and only the first -- which starts at
    the world's very first step, where nothing is re-ordered -- holds no re-ordering launch.  The later ones must not replay it."""
    assert M.reorder_points(REPLAY_CALLS, EVERY, "step") == [[], [3], [6], [9]]
    run_cadence(specs, form, True, 1, REPLAY_CALLS)
