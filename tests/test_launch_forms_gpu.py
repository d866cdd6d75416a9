"""Every launch form of the host layer (csrc/rem2d.hip: which kernels a step call enqueues, and what it times) with timing off and
on (pytest -m gpu): the same state either way, and exactly the launches / env-steps the read-back exports have always reported.

A launch form is a launch option (pipeline, fuse_velpost) and a tile shape; no result depends on it -- the parity suite holds the
forms to the oracle.  What is pinned HERE is the bookkeeping around the kernels: rem2d_world_enable_timing makes the group's first
world bracket the dominant kernel of every launch (rem2d_world_kernel_time_ms) and, on the tile pipeline, every env-step's whole
sequence (rem2d_world_step_time_ms); a timed launch goes through another launch call than an untimed one and must be the same
kernel on the same arguments.  The counts below were read from the launch code and confirmed on the library as it was before its
launch table (profiles/host_launch_refactor.txt).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CALLS = (1, 3, 7)            # step calls of one run: 11 env-steps in 3 calls
STEPS = sum(CALLS)
CONTINUOUS, DISCRETE = 1, 0  # REM2D_FLAG_CONTINUOUS

# (id, world flags, launch options, forced tile shape, launch_info() it must name, timed kernel launches, timed env-steps)
FORMS = [("fused-discrete", DISCRETE, {"pipeline": 0}, None, (-1, 0), len(CALLS), 0),      # n steps of a call in ONE launch
         ("fused-continuous", CONTINUOUS, {"pipeline": 0}, None, (-1, 0), STEPS, 0)]       # one launch per step: the TOI kernels follow
FORMS += [("tiles-shape%d" % s, CONTINUOUS, {"fuse_velpost": 0}, s, (s, 0), STEPS, STEPS) for s in range(5)]
FORMS += [("velpost", CONTINUOUS, {"fuse_velpost": 1}, None, (3, 1), STEPS, STEPS),
          ("train", CONTINUOUS, {"fuse_velpost": 2}, None, (3, 2), len(CALLS), STEPS),
          ("train128-shape1", CONTINUOUS, {"fuse_velpost": 2}, 1, (1, 2), len(CALLS), STEPS),
          ("train128-shape4", CONTINUOUS, {"fuse_velpost": 2}, 4, (4, 2), len(CALLS), STEPS)]


@pytest.fixture(scope="module")
def specs():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import synthetic
    return synthetic.lsystem_specs(range(96), mutate_odd=True)   # >= 3 lane buckets: the smallest population with a merged launch


def _run(specs, flags, options, shape, timing, rebalance=0, graph=False):
    """One population through CALLS: (state, [(kernel ms, launches, step ms, env-steps) per world, the group's first world first],
    the same read again, launch_info())."""
    import torch
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D(seed=4, flags=flags, options=options)
    env.tile_shape, env.rebalance_every, env.use_graph = shape, rebalance, graph
    env.reset_specs(specs)
    assert len(env.worlds) >= 3 and len(env.groups) == 1
    worlds = [env.worlds[i][0] for i in env.groups[0]]
    if timing:
        for w in worlds:
            w.enable_timing(True)
    info = env.launch_info()
    for n in CALLS:
        env.step(n)
    torch.cuda.synchronize()
    state = {"fitness": env.fitness.cpu().numpy(), "steps": env.steps.cpu().numpy(), "err": env.errors().cpu().numpy()}
    for k, w in enumerate(worlds):
        state["bodies%d" % k] = w.bodies()
        state["cn0_%d" % k] = w.view("cn0").cpu().numpy()
    reads = [[w.kernel_time_ms() + w.step_time_ms() for w in worlds] for _ in range(2)]
    env.close()
    return state, reads[0], reads[1], info


def _check(specs, flags, options, shape, want_info, launches, steps, **kw):
    off, first_off, _, info_off = _run(specs, flags, options, shape, False, **kw)
    on, first, second, info_on = _run(specs, flags, options, shape, True, **kw)
    print("launch_info", info_on, "first world", first[0], "others", first[1:], "second read", second[0])
    assert info_off == want_info and info_on == want_info
    assert off.keys() == on.keys()
    for name in off:   # (== on floats: a NaN anywhere fails, as it should)
        assert off[name].shape == on[name].shape and bool((off[name] == on[name]).all()), name
    assert bool((on["steps"] == STEPS).all()) and int(on["err"].max()) == 0
    kms, n_launches, sms, n_steps = first[0]
    assert (n_launches, n_steps) == (launches, steps)
    assert kms > 0 and (sms > 0) == (steps > 0)
    assert all(r == (0.0, 0, 0.0, 0) for r in first[1:])         # only the group's first world records
    assert all(r == (0.0, 0, 0.0, 0) for r in second)            # a read-back empties what it reports
    assert all(r == (0.0, 0, 0.0, 0) for r in first_off)         # timing off: nothing recorded at all


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_launch_form_same_state_and_exact_counts(specs, form):
    _, flags, options, shape, info, launches, steps = form
    _check(specs, flags, options, shape, info, launches, steps)


def test_train_is_cut_where_a_reordering_is_due(specs):
    """rebalance_every = 2 on the step train: a call longer than 2 steps goes in launches of at most 2 (tiles_launch_train's segment
    rule: 1 | 2 1 | 2 2 2 1), each with its own kernel pair and its own step bracket of that many env-steps."""
    _check(specs, CONTINUOUS, {"fuse_velpost": 2}, None, (3, 2), 1 + 2 + 4, STEPS, rebalance=2)


def test_timing_sends_a_graph_call_down_the_plain_enqueue(specs):
    """use_graph on per-step launches: with timing on nothing is captured (a replay would record no event), the counts are the
    per-step ones -- and the state equals the replayed (timing off) run's."""
    _check(specs, CONTINUOUS, {"fuse_velpost": 1}, None, (3, 1), STEPS, STEPS, graph=True)
