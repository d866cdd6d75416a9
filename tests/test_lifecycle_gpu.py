"""World reuse on the GPU (pytest -m gpu): a world that has lived through an episode, been scribbled on and reset must be the world
a fresh one is -- in every byte of every field over all padded rows right after the reset (the twin's image, BEFORE any step
runs) and after the next episode; so must a world created on an arena full of garbage, a world whose handle carries a leftover
creature order / error bits / a captured graph, and a world whose handle-owned scratch is a recycled block.

Modular2DEnv.py's gym idiom is ``env.reset()`` on one env object once per individual, and an EA run re-creates worlds for hundreds
of generations in one process; every other GPU test steps a world created a moment earlier on zeroed memory and resets it once.
Populations, dirt, field walker and the reference (the host-pointer twin's arena and oracle.batch_run) come from
tests/lifecycle_forge.py; tests/test_lifecycle_host.py holds the twin itself to the same statements.  `==` everywhere.
"""
import ctypes as C

import numpy as np
import pytest

import lifecycle_forge as F

pytestmark = pytest.mark.gpu

CONT = F.FLAG_CONTINUOUS


@pytest.fixture(scope="module")
def need_gpu():
    import replay
    replay.need_gpu()


@pytest.fixture(scope="module")
def ref(need_gpu, oracle, rough_terrain):
    """reference(lanes, flags): twin image, twin state and oracle run of P2, made once per (bucket, flags)."""
    return lambda lanes, flags=CONT: F.reference(lanes, flags, rough_terrain, oracle)


def _world(lanes, terrain, flags=CONT, wide=False, options=None):
    from gym_rem2d_amd.world import BatchedWorld
    w = BatchedWorld(F.N_ENVS[lanes], lanes, flags=flags, wide=wide, options=options)
    w.set_terrain(terrain)
    return w


def _episode1(w, m1, tile_shape=None):
    w.reset(m1, tile_shape=tile_shape)
    w.step(F.EPISODE1)
    F.scribble(w)


def _episode2(w):
    for n in F.EPISODE2_CALLS:
        w.step(n)


def _assert_image(w, image, what):
    """Right after a reset, before anything steps: every field over all padded rows == the twin's image."""
    assert F.differing(F.field_bytes(w), F.widen_image(image, w)) == [], what


def _assert_episode2(w, r, what, steps=F.EPISODE2):
    got = F.host_views(w)
    F.assert_like_oracle(got, r["after"] if steps == F.EPISODE2 else r["after30"], what)
    F.assert_like_batch_run(got, r["run"] if steps == F.EPISODE2 else r["run30"], what)
    assert int(got["err"].max()) == 0 and int(got["steps"].min()) == steps and w.handover_failures() == 0, what


# (id, launch options, build, tile shape of the FIRST reset, tile shape of the SECOND reset, compare with the twin / the oracle)
FORMS = [("train", None, False, None, None, True),
         ("velpost", {"fuse_velpost": 1}, False, None, None, True),
         ("two-launches", {"fuse_velpost": 0}, False, None, None, True),
         ("fused", {"pipeline": 0}, False, None, None, True),
         ("to-shape1", None, False, None, 1, True),           # the tile plan (and the launch form: train -> train128) changes
         ("to-shape4", None, False, None, 4, True),           # between the episodes
         ("to-shape0", None, False, None, 0, True),           # (train -> per-step launches of 256-body tiles)
         ("train128", None, False, 1, None, True),            # the 128-lane step train in both episodes
         ("wide", None, True, None, None, True),
         ("fma", None, "fma", None, None, False)]             # the tolerance-mode build: A versus B only


@pytest.mark.parametrize("lanes", F.LANES)
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_re_reset_equals_a_fresh_world(ref, rough_terrain, form, lanes):
    """a. World A: reset(P1), 120 steps, scribble, reset(P2).  World B: reset(P2).  After the reset every field of A over all padded
    rows == B's == the twin's image; only then both step 1 + 9 + 50, after which every field of A == B's in every byte (padding and
    empty lanes included) and both == the oracle (bodies, impulses, pair lists, reward, done, everdone, fitness)."""
    import torch
    name, options, build, shape1, shape2, with_oracle = form
    m1, m2 = F.populations(lanes)
    r = ref(lanes)
    a, b = (_world(lanes, rough_terrain, wide=build, options=options) for _ in range(2))
    _episode1(a, m1, tile_shape=shape1)
    assert int(a.view("steps").max()) == 7 and int(a.view("err").min()) == 1   # (the scribble is in place)
    shape2 = shape1 if shape2 is None else shape2
    a.reset(m2, tile_shape=shape2)
    b.reset(m2, tile_shape=shape2)
    torch.cuda.synchronize()
    fa, fb = F.field_bytes(a), F.field_bytes(b)
    assert F.differing(fa, fb) == [], "re-reset differs from a fresh reset"
    if with_oracle:
        _assert_image(a, r["image"], "reset image")
    _episode2(a)
    _episode2(b)
    torch.cuda.synchronize()
    assert F.differing(F.field_bytes(a), F.field_bytes(b)) == [], "episode 2 of the reused world differs from the fresh world's"
    if with_oracle:
        _assert_episode2(a, r, "reused")
        _assert_episode2(b, r, "fresh")
    else:
        assert int(a.view("err").max()) == 0 and int(a.view("steps").min()) == F.EPISODE2
    a.close()
    b.close()


@pytest.mark.parametrize("lanes", F.LANES)
@pytest.mark.parametrize("leftover", ["set-order", "rebalance", "retile", "skip-frozen"])
def test_leftover_order_is_harmless(ref, rough_terrain, leftover, lanes):
    """b. The handle keeps its creature order across a reset -- installed by the host, made by REM2D_OPT_REBALANCE from episode 1's
    position iterations, re-dealt by REM2D_FLAG_RETILE (both halves and the two fill counts) -- and, under REM2D_FLAG_SKIP_FROZEN,
    the "skip this creature" marks of blocks that had stopped.  Episode 2 == the oracle, no error bit."""
    import torch
    m1, m2 = F.populations(lanes)
    flags = CONT | {"retile": F.FLAG_RETILE, "skip-frozen": F.FLAG_SKIP_FROZEN}.get(leftover, 0)
    r = ref(lanes, flags & ~F.FLAG_RETILE)    # (a launch shape the twin ignores)
    w = _world(lanes, rough_terrain, flags=flags, options={"rebalance": 7} if leftover == "rebalance" else None)
    w.reset(m1)
    w.step(F.EPISODE1 // 2)
    if leftover == "set-order":
        w.set_order(torch.randperm(w.n_envs, generator=torch.Generator().manual_seed(lanes)))
    w.step(F.EPISODE1 - F.EPISODE1 // 2)
    F.scribble(w)
    if leftover == "skip-frozen":
        w.step(3)                             # every creature is `frozen` now: the blocks without padding stop and are marked as skipped
        assert int(w.view("steps").min()) == 7
    w.reset(m2)
    torch.cuda.synchronize()
    _assert_image(w, r["image"], leftover)
    _episode2(w)
    torch.cuda.synchronize()
    _assert_episode2(w, r, leftover)
    w.close()


def test_error_bits_and_failure_counter_do_not_leak(ref, rough_terrain):
    """c. Episode 1 holds the five-child hub (schedule period 5), which sets REM2D_ERR_SOLVER_OVERFLOW on its tile in the default
    build.  After reset(P2) `err` is 0 on every row, padding included, the hand-over failure counter is 0 and episode 2 == the
    oracle."""
    import torch
    from gym_rem2d_amd import _lib
    lanes = 8
    _, m2 = F.populations(lanes)
    r = ref(lanes)
    w = _world(lanes, rough_terrain)
    w.reset(F.hub_population(lanes))
    w.step(F.EPISODE1)
    err = w.view("err").cpu().numpy()
    assert err[1] & _lib.ERR_SOLVER_OVERFLOW, err     # (the hub, and with it the creatures that share its velocity tile)
    w.reset(m2)
    torch.cuda.synchronize()
    assert not np.frombuffer(F.field_bytes(w)["err"], dtype=np.int32).any()
    assert w.handover_failures() == 0
    _assert_image(w, r["image"], "after the hub")
    _episode2(w)
    torch.cuda.synchronize()
    _assert_episode2(w, r, "after the hub")
    w.close()


def _pattern(kind, n):
    import torch
    if kind == "random":
        return torch.from_numpy(np.random.default_rng(29).integers(0, 256, n, dtype=np.uint8))
    return torch.full((n,), {"ff": 0xFF, "7f": 0x7F}[kind], dtype=torch.uint8)


@pytest.mark.parametrize("lanes", F.LANES)
@pytest.mark.parametrize("kind", ["ff", "7f", "random"])
def test_dirty_arena(ref, rough_terrain, kind, lanes):
    """d. rem2d_world_create writes nothing into the arena it is given (asserted: the pattern put there BEFORE create is intact
    until reset), so a caller may hand over memory that holds anything: all-ones words (NaNs, index -1), 0x7f7f7f7f (huge finite
    floats, huge indices), random bytes.  reset(P2) must make every field over all padded rows == the twin's image -- asserted
    before any step runs: a field the reset missed fails here and never reaches a kernel.  Then 60 steps == a fresh world's on a
    zeroed arena == the oracle's, and every alignment-gap byte still holds the pattern: no kernel writes outside a field."""
    import torch
    _, m2 = F.populations(lanes)
    r = ref(lanes)
    w = _world(lanes, rough_terrain)
    pattern = _pattern(kind, w.arena.numel())
    w.arena.copy_(pattern)
    F.recreate_on(w, w.arena)
    w.set_terrain(rough_terrain)
    assert np.array_equal(F.arena_bytes(w), pattern.numpy()), "create / set_terrain wrote into the arena"
    w.reset(m2)
    torch.cuda.synchronize()
    _assert_image(w, r["image"], kind)        # BEFORE any step
    b = _world(lanes, rough_terrain)
    b.reset(m2)
    _episode2(w)
    _episode2(b)
    torch.cuda.synchronize()
    assert F.differing(F.field_bytes(w), F.field_bytes(b)) == []
    _assert_episode2(w, r, kind)
    after, gaps = F.arena_bytes(w), F.gaps(w)
    assert gaps
    for lo, hi in gaps:
        assert np.array_equal(after[lo:hi], pattern.numpy()[lo:hi]), ("gap", lo, hi)
    w.close()
    b.close()


def test_guard_bytes_around_a_caller_owned_arena(ref, rough_terrain):
    """d, additionally: a world created through the ABI inside a test-owned tensor, 256-byte aligned, with 4 KiB of pattern in front
    of and behind the rem2d_state_bytes window.  Both guards are intact after reset + 60 steps, and the result == the oracle."""
    import torch
    lanes = 4
    _, m2 = F.populations(lanes)
    r = ref(lanes)
    w = _world(lanes, rough_terrain)
    nbytes = w.arena.numel()
    assert nbytes == w.L.rem2d_state_bytes(C.byref(w.cfg))
    guard = 4096
    big = torch.from_numpy(np.random.default_rng(31).integers(0, 256, nbytes + 2 * guard + 256, dtype=np.uint8)).cuda()
    lo = guard + (-(big.data_ptr() + guard)) % 256
    want = big.cpu().numpy()
    F.recreate_on(w, big[lo:lo + nbytes])
    w.set_terrain(rough_terrain)
    w.reset(m2)
    torch.cuda.synchronize()
    _assert_image(w, r["image"], "guarded")
    _episode2(w)
    torch.cuda.synchronize()
    _assert_episode2(w, r, "guarded")
    got = big.cpu().numpy()
    assert lo >= guard and big.numel() - (lo + nbytes) >= guard
    assert np.array_equal(got[:lo], want[:lo]), "bytes in front of the arena were written"
    assert np.array_equal(got[lo + nbytes:], want[lo + nbytes:]), "bytes behind the arena were written"
    w.close()


def test_graph_replay_across_a_reset(ref, rough_terrain):
    """e. rem2d_world_reset does not invalidate a captured graph (nothing the kernel arguments embed changes).  Two worlds as one
    step group through rem2d_groups_step with REM2D_STEP_GRAPH, on per-step launches (a step train is never captured): 10 + 10
    steps of P1 capture and replay the call, rem2d_world_reset(P2) alone on both (no new tile table: the replay key stays), then
    10 + 10 + 10 replayed steps == the oracle at 30 steps."""
    import torch
    from gym_rem2d_amd import _lib
    worlds = [_world(k, rough_terrain, options={"fuse_velpost": 1}) for k in F.LANES]
    arr = _lib.world_array(worlds)
    group = (_lib.StepGroup * 1)()
    group[0].worlds, group[0].n_worlds, group[0].stream = C.cast(arr, C.POINTER(C.c_void_p)), len(worlds), None

    def step(n):
        _lib.check(_lib.lib().rem2d_groups_step(group, 1, n, worlds[0]._stream(), _lib.STEP_GRAPH))
    for w in worlds:
        F.raw_reset(w, F.populations(w.lanes)[0])
    step(10)
    step(10)
    for w in worlds:
        assert int(w.view("steps").min()) == 20
        F.scribble(w)
        F.raw_reset(w, F.populations(w.lanes)[1])
    torch.cuda.synchronize()
    for w in worlds:
        _assert_image(w, ref(w.lanes)["image"], "graph")
    for n in F.GRAPH_CALLS:
        step(n)
    torch.cuda.synchronize()
    for w in worlds:
        _assert_episode2(w, ref(w.lanes), "graph", steps=sum(F.GRAPH_CALLS))
        w.close()


def test_env_tier_reset_batches_twice(ref, rough_terrain):
    """f. BatchedModular2D.reset_batches(P1 buckets), 120 steps, reset_batches(P2 buckets), 60 steps: the worlds of the second
    population are created right after the first ones' were destroyed (their scratch is what the allocator hands back).  Fitness,
    reward and done in population order == a fresh env's == the oracle's."""
    import torch
    from gym_rem2d_amd.env import BatchedModular2D
    n4 = F.N_ENVS[4]
    index = {4: list(range(n4)), 8: list(range(n4, n4 + F.N_ENVS[8]))}

    def batches(which):
        return [(F.populations(k)[which], index[k]) for k in F.LANES]

    def read(env):
        reward, done = env._reward, env._done
        torch.cuda.synchronize()
        assert int(env.errors().max()) == 0
        return env.fitness.cpu().numpy(), reward.cpu().numpy().copy(), done.cpu().numpy().copy()
    env = BatchedModular2D(seed=4, flags=CONT)
    env.reset_batches(batches(0))
    assert len(env.worlds) >= 2
    env.step(F.EPISODE1)
    env.reset_batches(batches(1))
    for n in F.EPISODE2_CALLS:
        env.step(n)
    reused = read(env)
    env.close()
    fresh_env = BatchedModular2D(seed=4, flags=CONT)
    fresh_env.reset_batches(batches(1))
    for n in F.EPISODE2_CALLS:
        fresh_env.step(n)
    fresh = read(fresh_env)
    fresh_env.close()
    for a, b in zip(reused, fresh):
        assert np.array_equal(a, b)
    for k in F.LANES:
        run = ref(k)["run"]
        assert np.array_equal(reused[0][index[k]], run["fitness"])
        assert np.array_equal(reused[1][index[k]], run["reward"].astype(np.float32))
        last = ref(k)["after"]["done"] != 0     # (done of the LAST step: the twin's; batch_run reports "ever done")
        assert np.array_equal(reused[2][index[k]], last)


def test_gym_facade_reset_twice(need_gpu):
    """f. Modular2D, the reference's idiom: reset(tree1), 80 steps, reset(tree2), 80 steps on ONE env object.  Observations (closed
    loop, so that there are some) and rewards of the second episode == those of a fresh Modular2D given tree2."""
    import random
    from gym_rem2d_amd.encodings import LSystem
    from gym_rem2d_amd.env import Modular2D
    from gym_rem2d_amd.modules import get_module_list

    def tree(seed):
        random.seed(seed)
        ml = get_module_list()
        return LSystem(ml).create(8), ml

    def episode(env, seed):
        t, ml = tree(seed)
        out = [env.reset(tree=t, module_list=ml)]
        rewards = []
        for _ in range(80):
            obs, reward, done, _ = env.step(None)
            out.append(obs)
            rewards.append((reward, done))
        return np.stack(out), rewards
    env = Modular2D(closed_loop=True)
    env.seed(4)
    first = episode(env, 2)
    second = episode(env, 15)
    env.close()
    fresh_env = Modular2D(closed_loop=True)
    fresh_env.seed(4)
    fresh = episode(fresh_env, 15)
    fresh_env.close()
    assert first[0].shape == second[0].shape and not np.array_equal(first[0], second[0])
    assert second[0].tobytes() == fresh[0].tobytes()
    assert second[1] == fresh[1]


def test_release_then_create_the_same_shape(ref, rough_terrain):
    """f. Create and step a lanes-8 world with P1, release() it, create a world of the same shape at once and run P2 on it: its
    scratch block is the size of the one just freed.  OPPORTUNISTIC: hipMalloc may or may not hand the old block back, so this id
    only meets a recycled scratch when the allocator does; the deterministic checks of the scratch are the re-reset tests above
    (a world that keeps its own used scratch)."""
    import torch
    lanes = 8
    m1, m2 = F.populations(lanes)
    r = ref(lanes)
    w = _world(lanes, rough_terrain)
    w.reset(m1)
    w.step(F.EPISODE1)
    torch.cuda.synchronize()
    w.release()
    w = _world(lanes, rough_terrain)
    w.reset(m2)
    _episode2(w)
    torch.cuda.synchronize()
    _assert_episode2(w, r, "recycled")
    w.close()
