"""The worlds BatchedModular2D builds are the worlds launch_policy.plan planned (pytest -m gpu): shapes, flags, options, tile
shapes and population indices of the real worlds against the plan object, the library's own launch form against the plan's train
flag, results against a default env, and compact()'s new worlds against the same plan."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def population():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import synthetic
    batches = synthetic.lsystem_batches_native(range(96))   # 40 / 13 / 10 / 33 creatures on 2 / 4 / 8 / 16 lanes
    assert len(batches) > 1
    n = sum(m.n_envs for m, _ in batches)
    from gym_rem2d_amd.env import BatchedModular2D
    ref = BatchedModular2D()   # one group, default constants
    ref._upload(batches, n)
    ref.step(3)
    want = ref.fitness.clone(), ref.steps.clone(), ref.errors().clone()
    ref.close()
    return batches, n, want


# 256: three groups' shares of these buckets still fit one world each (at most 12 creatures of 16 lanes); 64: the 8- and 16-lane
# buckets are cut into two and three worlds a group
@pytest.mark.parametrize("max_world_lanes", [256, 64])
def test_worlds_built_are_the_worlds_planned(population, max_world_lanes):
    import torch
    from gym_rem2d_amd import _lib
    from gym_rem2d_amd.env import BatchedModular2D
    batches, n, (fitness, steps, errors) = population
    env = BatchedModular2D()
    env.step_groups = 3
    env.MAX_WORLD_LANES = max_world_lanes
    env._upload(batches, n)
    plan = env._plan
    forced = _lib.env_options()   # (the suite is also run with launch options forced: every world gets them below the plan's)
    options = dict(forced, **(plan.world_options or {}))

    def shape(chosen):
        return chosen if chosen is not None else (_lib.env_tile_shape() if _lib.env_tile_shape() is not None else -1)

    assert len(env.worlds) == len(plan.pieces) and plan.groups == 3
    assert len(env.worlds) > 3 * len(batches) or max_world_lanes == 256
    for (w, idx), p in zip(env.worlds, plan.pieces):
        m, pop_idx = batches[p.bucket]
        assert (w.n_envs, w.lanes, w.flags) == (len(p.members), m.lanes, plan.world_flags)
        assert w.get_option("fuse_velpost") == options.get("fuse_velpost", 2)   # (2: the library's default, the step train)
        assert w.get_option("rebalance") == options.get("rebalance", 0)
        assert w.tile_shape == shape(plan.tile_shape_by_lanes.get(m.lanes, plan.tile_shape))
        assert np.array_equal(idx.cpu().numpy(), np.asarray(pop_idx)[p.members])
    assert [[env.worlds[i][0].lanes for i in g] for g in env.groups] == \
        [[batches[p.bucket][0].lanes for p in plan.pieces if p.group == g] for g in range(3)]
    assert (env.launch_info()[1] == 2) == plan.train

    env.step(3)   # results never depend on the launch form
    assert torch.equal(env.fitness, fitness) and torch.equal(env.steps, steps) and torch.equal(env.errors(), errors)

    # compact(): the world that takes a bucket's survivors is made from the same plan
    for w, _ in env.worlds:   # (nobody's fitness is final after three steps: every other creature's is closed by hand)
        w.view("frozen")[::2] = 1
    alive = env.compact(min_envs=1)
    assert 0 < alive <= n // 2
    new = [w for wi, (w, _) in enumerate(env.worlds) if wi not in env._inactive]
    assert sorted(w.lanes for w in new) == [m.lanes for m, _ in batches] and sum(w.n_envs for w in new) == alive
    for w in new:
        assert w.flags == plan.world_flags and w.tile_shape == shape(plan.tile_shape)
        assert w.get_option("fuse_velpost") == options.get("fuse_velpost", 2)
        assert w.get_option("rebalance") == options.get("rebalance", 0)
    env.step(1)
    assert int(env.steps.max()) == 4
    env.close()
