"""The launch policy (gym_rem2d_amd/launch_policy.py) pinned on the CPU to the _upload it was cut out of.

tests/golden/launch_plans.json is what tools/record_launch_plans.py recorded from the commit before the planner existed: for every
case of its CASES, what BatchedModular2D._upload decided (groups, tile shape, launch options, world flags, rebalance period) and
which worlds it built in which order, with a stand-in for BatchedWorld.  Every case is held to it twice: the planner alone, fed
the case's bucket records, knobs and overrides; and this tree's _upload with the same stand-in.  Which branch of the policy a case
is there for is its `branch` (record_launch_plans.BRANCHES spells the names out; test_every_branch_has_a_case lists them).
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_launch_plans as R  # noqa: E402

from gym_rem2d_amd import _lib, launch_policy  # noqa: E402
from gym_rem2d_amd import env as envmod  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "launch_plans.json")) as f:
    RECORDED = json.load(f)


@pytest.fixture
def case_env(monkeypatch):
    """Sets a case's environment: every REM2D_* launch override removed (the suite is also run with a shape forced), then the case's."""
    def set_up(c):
        for v in R.OVERRIDE_VARS:
            monkeypatch.delenv(v, raising=False)
        for k, v in c["env"].items():
            monkeypatch.setenv(k, v)
    return set_up


def test_every_branch_has_a_case():
    """The branches of the policy, and that CASES reaches each: the two group ladders, forced groups, the tile shape (population
    size, uniform populations, attribute, both overrides), train or per-step launches (TRAIN128_MAX, TRAIN128_UNIFORM, fuse_velpost
    given, pipeline / debug), the train's group count, retile, rebalance, the two group splits, world cutting, set_outputs."""
    assert set(R.BRANCHES) == {"bench", "ladder_short", "ladder_long", "forced_groups", "shape_big", "shape_uniform", "shape_attr",
                               "shape_env", "shape_by_lanes", "train128_max", "train128_uniform", "fuse_given", "no_train",
                               "train_groups", "retile", "rebalance", "group_split", "world_cut", "outputs"}
    reached = {b for c in R.CASES for b in c["branch"].split()}
    assert reached == set(R.BRANCHES)
    assert sorted(c["name"] for c in R.CASES) == sorted(RECORDED)
    # the full-size populations stay in the list
    sizes = {sum(b[0] for b in c["buckets"]) for c in R.CASES if "bench" in c["branch"].split()}
    assert {65536, 131072, 131073, 196608, 1048576} <= sizes


@pytest.mark.parametrize("c", R.CASES, ids=[c["name"] for c in R.CASES])
def test_planner_reproduces_the_recorded_plan(c, case_env):
    case_env(c)
    want = RECORDED[c["name"]]
    env = R.new_env(envmod, c)   # (no device needed: the constructor reads its four overrides, the case sets attributes)
    assert [env.merged_launch, env.step_groups, env.use_graph, env.rebalance_every] == want["public"]
    knobs = launch_policy.Knobs(env.step_groups, env.tile_shape, env.flags, env.options, env.rebalance_every, env.BIG_POPULATION,
                                env.TRAIN128_MAX, env.TRAIN128_UNIFORM, env.REBALANCE_EVERY, env.MAX_WORLD_LANES,
                                _lib.MAX_STEP_GROUPS, _lib.MAX_WORLDS_PER_STEP)
    buckets = [launch_policy.Bucket(*b) for b in c["buckets"]]
    n = sum(b.n_envs for b in buckets)
    plan = launch_policy.plan(buckets, n, knobs, launch_policy.read_overrides())

    assert plan.tile_shape == want["tile_shape_used"]
    assert sorted(plan.tile_shape_by_lanes.items()) == [tuple(x) for x in want["tile_shape_by_lanes"]]
    assert plan.launch_options == want["launch_options"]
    assert plan.world_flags == want["world_flags"]
    assert plan.rebalance_steps == want["rebalance_steps"]
    assert plan.eff_tile_shape == (plan.tile_shape if plan.tile_shape is not None else _lib.env_tile_shape())
    groups = [[] for _ in range(plan.groups)]
    for wi, p in enumerate(plan.pieces):
        groups[p.group].append(wi)
    groups = [g for g in groups if g]
    assert groups == want["groups"]
    group_of = {wi: g for g, ws in enumerate(groups) for wi in ws}
    index = [np.asarray(idx, dtype=np.int64) for _, idx in R.batches_of(c)[0]]   # the case's population index, bucket by bucket
    got = [{"n_envs": len(p.members), "lanes": buckets[p.bucket].lanes, "flags": plan.world_flags, "options": plan.world_options,
            "tile_shape": plan.tile_shape_by_lanes.get(buckets[p.bucket].lanes, plan.tile_shape), "group": group_of[wi],
            "index": R.sha(index[p.bucket][p.members], np.int64)} for wi, p in enumerate(plan.pieces)]
    assert all(p.members.dtype == np.int64 for p in plan.pieces)
    assert got == [{k: w[k] for k in got[0]} for w in want["worlds"]]
    # the train flag was a local of the recorded _upload; what it stands for can be said from the record: a train is the library's
    # default launch form (fuse_velpost 2) on the tile shapes that have one, with nothing that forbids it
    opts = dict(_lib.env_options(), **(plan.world_options or {}))
    assert plan.train == (plan.eff_tile_shape in (1, 3, 4) and c["env"].get("REM2D_RETILE") != "1"
                          and opts.get("fuse_velpost", 2) == 2 and opts.get("pipeline", 3) == 3 and opts.get("debug", 0) == 0)


@pytest.mark.parametrize("c", R.CASES, ids=[c["name"] for c in R.CASES])
def test_upload_builds_the_recorded_worlds(c, case_env):
    """This tree's _upload with the stand-in world: the same constructions, reset shapes, set_outputs calls, groups and attributes,
    in the same order."""
    case_env(c)
    assert R.jsonable(R.run_case(envmod, c)) == RECORDED[c["name"]]


def test_overrides_are_read_when_they_were(monkeypatch):
    """The four variables of the constructor land in the public attributes and are not read again; _upload's are read at each call."""
    for v in R.OVERRIDE_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in (("REM2D_MERGED_LAUNCH", "0"), ("REM2D_STEP_GROUPS", "3"), ("REM2D_GRAPH", "1"), ("REM2D_REBALANCE", "25")):
        monkeypatch.setenv(k, v)
    c = R.case("late", "forced_groups", R.mixed((50, 4), (100, 16)))
    env = R.new_env(envmod, c)
    assert (env.merged_launch, env.step_groups, env.use_graph, env.rebalance_every) == (False, 3, True, 25)
    for k in ("REM2D_MERGED_LAUNCH", "REM2D_STEP_GROUPS", "REM2D_GRAPH", "REM2D_REBALANCE"):
        monkeypatch.delenv(k)
    monkeypatch.setenv("REM2D_RETILE", "1")   # (set after construction: _upload sees it)
    rec = R.run_case(envmod, c)   # a new env, constructed without the four: the defaults
    assert rec["public"] == [True, 0, False, -1] and rec["world_flags"] & _lib.FLAG_RETILE
    assert (env.merged_launch, env.step_groups, env.use_graph, env.rebalance_every) == (False, 3, True, 25)
    over = launch_policy.read_overrides()
    assert over.retile and over.options == _lib.env_options() and over.tile_shape == _lib.env_tile_shape()
