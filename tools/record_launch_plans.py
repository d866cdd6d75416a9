#!/usr/bin/env python
"""Record what BatchedModular2D._upload decides and builds for a list of populations, without a GPU.

    python tools/record_launch_plans.py CHECKOUT [-o launch_plans.json]

imports gym_rem2d_amd from CHECKOUT (this tree, or a `git worktree` of another commit), replaces env.BatchedWorld by a stand-in
that records how it is constructed, reset and given its outputs, env.group_streams and the terrain by stubs, and runs every case
of CASES through that checkout's _upload.  tests/golden/launch_plans.json is the output for the commit before
gym_rem2d_amd/launch_policy.py existed (the policy still inside _upload); tests/test_launch_policy.py holds the planner and the
_upload of the tree it runs in to it.

A case: the lane buckets (n_envs, lanes, uniform) in upload order, constructor arguments, attributes set on the instance after
construction (class constants lowered there reach the thresholds at small sizes), REM2D_* variables, and the order of the
population index ("identity": bucket after bucket as bench.py uploads; "reversed": a population whose order is not the worlds').
`branch` names the branches of the policy the case is there for (BRANCHES).
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

# every variable the launch policy or a world reads; a case starts from an environment without any of them
OVERRIDE_VARS = ("REM2D_MERGED_LAUNCH", "REM2D_STEP_GROUPS", "REM2D_GRAPH", "REM2D_REBALANCE", "REM2D_SORT_DESC", "REM2D_TILE_SHAPE",
                 "REM2D_TILE_SHAPE_BY_LANES", "REM2D_TILE_CREATURES", "REM2D_RETILE", "REM2D_GROUP_SPLIT", "REM2D_PIPELINE",
                 "REM2D_FUSE_VELPOST", "REM2D_PRIO", "REM2D_PRIO_T1", "REM2D_PRIO_T2", "REM2D_HEAVY_PER_WAVE", "REM2D_V4_DBG",
                 "REM2D_REBALANCE_DEV", "REM2D_TRAIN_FAULT")

BRANCHES = {
    "bench": "the populations bench.py runs, at full size",
    "ladder_short": "group ladder of short steps (one lane bucket below 16 lanes): blocks < 3072, 3072 .. 6143, >= 6144",
    "ladder_long": "group ladder of long steps (two buckets, or lanes >= 16): blocks < 512, >= 512",
    "forced_groups": "step_groups forced to 1, 3, 4, with a bucket of n_envs < 4 * groups that is not split",
    "shape_big": "tile shape below and at BIG_POPULATION",
    "shape_uniform": "uniform population, blocks / groups at 2048 (shape 3) and just above (shape 4)",
    "shape_attr": "env.tile_shape set",
    "shape_env": "REM2D_TILE_SHAPE set",
    "shape_by_lanes": "REM2D_TILE_SHAPE_BY_LANES set",
    "train128_max": "shape 1 at and above TRAIN128_MAX",
    "train128_uniform": "shape 4 with TRAIN128_UNIFORM false and true",
    "fuse_given": "fuse_velpost given in options and via REM2D_FUSE_VELPOST",
    "no_train": "pipeline=0 and debug=1 disable the train",
    "train_groups": "the train's group count grows when worlds_per_group exceeds MAX_WORLDS_PER_STEP",
    "retile": "REM2D_RETILE=1: flags, rebalance period 0, no train",
    "rebalance": "rebalance period: automatic at 4095 / 4096 mixed creatures, uniform, REM2D_REBALANCE=0 / 25",
    "group_split": "round-robin and REM2D_GROUP_SPLIT=cut over lanes 4, 8, 16, 32 (run length 64 // lanes)",
    "world_cut": "MAX_WORLD_LANES lowered until a group's bucket needs two and three worlds",
    "outputs": "set_outputs: more than one world, or one world whose order is not the identity",
}

# lane buckets of bench.py's populations of 65 536 creatures (synthetic.lsystem_batches_native / cppn_batches_native of seeds
# 0 .. 65 535: (creatures, lanes)); the larger L-system populations are this mix scaled
LSYSTEM_65536 = ((26141, 2), (12056, 4), (4951, 8), (22388, 16))
CPPN_65536 = ((32926, 2), (11502, 4), (4249, 8), (4091, 16), (12768, 32))


def lsystem_mix(n):
    """LSYSTEM_65536 scaled to n creatures (the remainder goes to the last bucket)."""
    counts = [c * n // 65536 for c, _ in LSYSTEM_65536]
    counts[-1] += n - sum(counts)
    return [(c, lanes, False) for c, (_, lanes) in zip(counts, LSYSTEM_65536)]


def mixed(*buckets):
    return [(n, lanes, False) for n, lanes in buckets]


def case(name, branch, buckets, ctor=None, attrs=None, env=None, order="identity"):
    assert all(b in BRANCHES for b in branch.split()), branch
    return {"name": name, "branch": branch, "buckets": [tuple(b) for b in buckets], "ctor": ctor or {}, "attrs": attrs or {},
            "env": env or {}, "order": order}


PER_STEP = {"options": {"fuse_velpost": 1}}   # per-step launches: the automatic group count is not overridden by the train's
SMALL = {"BIG_POPULATION": 1000, "TRAIN128_MAX": 1000}
FIVE = mixed((101, 2), (77, 4), (50, 8), (37, 16), (29, 32))

CASES = [
    # ---- bench.py's populations ----
    case("lsystem_65536", "bench ladder_long rebalance outputs", [b + (False,) for b in LSYSTEM_65536]),
    case("lsystem_131072", "bench shape_big train128_max", lsystem_mix(131072)),
    case("lsystem_131073", "bench train128_max", lsystem_mix(131073)),
    case("lsystem_196608", "bench train128_max", lsystem_mix(196608)),
    case("lsystem_1048576", "bench", lsystem_mix(1048576)),
    case("cppn_65536", "bench ladder_long", [b + (False,) for b in CPPN_65536], ctor={"hardcore": True}),
    case("chain8_65536", "bench shape_uniform train128_uniform ladder_short", [(65536, 8, True)]),
    case("chain8_65536_train128_uniform", "train128_uniform", [(65536, 8, True)], attrs={"TRAIN128_UNIFORM": True}),
    case("chain4_65536", "bench shape_uniform", [(65536, 4, True)]),          # 4096 blocks, two groups: 2048 a group -> shape 3
    case("chain4_65552", "shape_uniform", [(65552, 4, True)]),                # 4097 blocks: 2048.5 a group -> shape 4
    # ---- the group ladders (on per-step launches, where the count stands) ----
    case("short_3071_blocks", "ladder_short", [(24568, 8, False)], ctor=PER_STEP),
    case("short_3072_blocks", "ladder_short", [(24576, 8, False)], ctor=PER_STEP),
    case("short_6143_blocks", "ladder_short", [(49144, 8, False)], ctor=PER_STEP),
    case("short_6144_blocks", "ladder_short", [(49152, 8, False)], ctor=PER_STEP),
    case("long_16_lanes_511_blocks", "ladder_long", [(2044, 16, False)], ctor=PER_STEP),
    case("long_16_lanes_512_blocks", "ladder_long", [(2048, 16, False)], ctor=PER_STEP),
    case("long_two_buckets_below_512", "ladder_long", mixed((4096, 4), (2047, 8)), ctor=PER_STEP),
    case("long_two_buckets_512", "ladder_long", mixed((4096, 4), (2048, 8)), ctor=PER_STEP),
    case("train_takes_one_group", "ladder_long outputs", mixed((4096, 4), (2048, 8))),
    # ---- forced groups ----
    case("forced_1", "forced_groups", mixed((4096, 4), (2048, 8)), ctor=PER_STEP, attrs={"step_groups": 1}),
    case("forced_3_unsplit_bucket", "forced_groups", mixed((11, 4), (12, 8), (100, 16)), attrs={"step_groups": 3}),
    case("forced_4_unsplit_bucket", "forced_groups", mixed((15, 4), (16, 8), (100, 16)), attrs={"step_groups": 4}),
    case("forced_3_by_environment", "forced_groups", mixed((50, 4), (100, 16)), env={"REM2D_STEP_GROUPS": "3"}),
    case("forced_4_only_first_group_used", "forced_groups outputs", [(9, 8, False)], attrs={"step_groups": 4}),
    # ---- tile shape ----
    case("below_big_population", "shape_big", mixed((600, 4), (399, 8)), attrs=SMALL),
    case("at_big_population", "shape_big train128_max", mixed((600, 4), (400, 8)), attrs=SMALL),
    case("above_train128_max", "train128_max", mixed((600, 4), (401, 8)), attrs=SMALL),
    case("train128_max_below_big", "train128_max", mixed((600, 4), (401, 8)), attrs={"BIG_POPULATION": 1000, "TRAIN128_MAX": 500}),
    case("tile_shape_attr_0", "shape_attr", mixed((600, 4), (400, 8)), attrs={"tile_shape": 0}),
    case("tile_shape_attr_1", "shape_attr", mixed((600, 4), (400, 8)), attrs={"tile_shape": 1}),
    case("tile_shape_attr_4_mixed", "shape_attr train128_uniform", mixed((600, 4), (400, 8)), attrs={"tile_shape": 4}),
    case("tile_shape_attr_4_train", "shape_attr train128_uniform", mixed((600, 4), (400, 8)),
         attrs={"tile_shape": 4, "TRAIN128_UNIFORM": True}),
    case("tile_shape_env_2", "shape_env", mixed((600, 4), (400, 8)), env={"REM2D_TILE_SHAPE": "2"}),
    case("tile_shape_env_1_above_train128_max", "shape_env train128_max", mixed((600, 4), (401, 8)), attrs=SMALL,
         env={"REM2D_TILE_SHAPE": "1"}),
    case("tile_shape_env_4", "shape_env train128_uniform", [(5000, 8, True)], env={"REM2D_TILE_SHAPE": "4"}),
    case("tile_shape_attr_beats_env", "shape_attr shape_env", mixed((600, 4), (400, 8)), attrs={"tile_shape": 3},
         env={"REM2D_TILE_SHAPE": "0"}),
    case("tile_shape_by_lanes", "shape_by_lanes", FIVE, env={"REM2D_TILE_SHAPE_BY_LANES": "2:1,4:1,32:0"}),
    # ---- train or per-step launches ----
    case("fuse_velpost_2_in_options", "fuse_given", mixed((600, 4), (401, 8)), ctor={"options": {"fuse_velpost": 2}}, attrs=SMALL),
    case("fuse_velpost_0_in_options", "fuse_given", mixed((600, 4), (400, 8)), ctor={"options": {"fuse_velpost": 0}}),
    case("fuse_velpost_1_by_environment", "fuse_given", mixed((4096, 4), (2048, 8)), env={"REM2D_FUSE_VELPOST": "1"}),
    case("fuse_velpost_2_by_environment", "fuse_given", mixed((600, 4), (401, 8)), attrs=SMALL, env={"REM2D_FUSE_VELPOST": "2"}),
    case("options_beat_environment", "fuse_given", mixed((4096, 4), (2048, 8)), ctor={"options": {"fuse_velpost": 2}},
         env={"REM2D_FUSE_VELPOST": "1"}),
    case("pipeline_0_in_options", "no_train", mixed((4096, 4), (2048, 8)), ctor={"options": {"pipeline": 0}}),
    case("pipeline_0_by_environment", "no_train", mixed((4096, 4), (2048, 8)), env={"REM2D_PIPELINE": "0"}),
    case("debug_1_in_options", "no_train", mixed((4096, 4), (2048, 8)), ctor={"options": {"debug": 1}}),
    case("debug_1_by_environment", "no_train", mixed((4096, 4), (2048, 8)), env={"REM2D_V4_DBG": "1"}),
    # ---- the train's group count ----
    case("train_8_worlds_one_group", "train_groups world_cut", mixed((256, 4), (448, 16)), attrs={"MAX_WORLD_LANES": 1024}),
    case("train_9_worlds_two_groups", "train_groups world_cut", mixed((257, 4), (448, 16)), attrs={"MAX_WORLD_LANES": 1024}),
    case("train_three_groups", "train_groups world_cut", mixed((600, 8), (1000, 16)), attrs={"MAX_WORLD_LANES": 1024}),
    case("train_groups_at_the_limit", "train_groups world_cut", [(200, 16, False)], attrs={"MAX_WORLD_LANES": 16}),
    # ---- retile, flags ----
    case("retile", "retile", mixed((4096, 4), (2048, 8)), env={"REM2D_RETILE": "1"}),
    case("retile_flag_of_the_caller_is_dropped", "retile", mixed((600, 4), (400, 8)), ctor={"flags": 1 | 8 | 16}),
    case("discrete_wide", "retile", mixed((600, 4), (400, 8)), ctor={"flags": 0, "wide": True}),
    # ---- rebalance ----
    case("mixed_4095", "rebalance", mixed((4000, 4), (95, 8))),
    case("mixed_4096", "rebalance", mixed((4000, 4), (96, 8))),
    case("uniform_8192", "rebalance", [(8192, 8, True)]),
    case("one_uniform_bucket_of_two", "rebalance", [(4000, 4, True), (96, 8, False)]),
    case("rebalance_0_by_environment", "rebalance", mixed((4000, 4), (96, 8)), env={"REM2D_REBALANCE": "0"}),
    case("rebalance_25_by_environment", "rebalance", mixed((600, 4), (400, 8)), env={"REM2D_REBALANCE": "25"}),
    case("rebalance_every_attr", "rebalance", [(8192, 8, True)], attrs={"rebalance_every": 10}),
    case("rebalance_in_options", "rebalance", mixed((4000, 4), (96, 8)), ctor={"options": {"rebalance": 7}}),
    case("rebalance_default_lowered", "rebalance", mixed((4000, 4), (96, 8)), attrs={"REBALANCE_EVERY": 20}),
    # ---- group split ----
    case("round_robin", "group_split", FIVE, attrs={"step_groups": 3}),
    case("cut", "group_split", FIVE, attrs={"step_groups": 3}, env={"REM2D_GROUP_SPLIT": "cut"}),
    case("round_robin_reversed_population", "group_split outputs", FIVE, attrs={"step_groups": 4}, order="reversed"),
    # ---- world cutting ----
    case("two_worlds_a_group", "world_cut", [(100, 8, False)], attrs={"step_groups": 2, "MAX_WORLD_LANES": 256}),
    case("three_worlds_a_group", "world_cut", [(100, 8, False)], attrs={"step_groups": 2, "MAX_WORLD_LANES": 160}),
    case("wider_than_max_world_lanes", "world_cut", [(5, 32, False)], attrs={"MAX_WORLD_LANES": 16}),
    # ---- set_outputs ----
    case("one_world_identity", "outputs", [(300, 8, False)]),
    case("one_world_reversed", "outputs", [(300, 8, False)], order="reversed"),
    case("one_creature", "outputs", [(1, 2, True)]),
]


class StandInMorph:
    """As much of a Morphology as _upload and the `_uniform` predicate touch: the three int arrays, take()."""

    def __init__(self, n_envs, lanes, uniform=True, arrays=None):
        self.n_envs, self.lanes = int(n_envs), int(lanes)
        if arrays is None:
            arrays = {"shape": np.ones(n_envs * lanes, np.int8), "parent": np.full(n_envs * lanes, -1, np.int8),
                      "jround": np.zeros(n_envs * lanes, np.int8)}
            if not uniform:
                arrays["jround"][::lanes] = np.arange(n_envs) % 2 == 0
        self.arrays = arrays

    def take(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        lanes = (idx[:, None] * self.lanes + np.arange(self.lanes)[None, :]).reshape(-1)
        return StandInMorph(len(idx), self.lanes, arrays={k: v[lanes] for k, v in self.arrays.items()})


def batches_of(c):
    """[(morph, population index)] of a case, as _upload takes them, and the population size."""
    n = sum(b[0] for b in c["buckets"])
    out, lo = [], 0
    for n_envs, lanes, uniform in c["buckets"]:
        idx = np.arange(lo, lo + n_envs)
        out.append((StandInMorph(n_envs, lanes, uniform), (n - 1 - idx if c["order"] == "reversed" else idx).tolist()))
        lo += n_envs
    return out, n


def sha(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a), dtype=dtype).tobytes()).hexdigest()


def new_env(envmod, c):
    """The BatchedModular2D of a case (the environment is the case's already: the constructor reads four variables)."""
    env = envmod.BatchedModular2D(**c["ctor"])
    for k, v in c["attrs"].items():
        setattr(env, k, v)
    return env


def run_case(envmod, c):
    """Run case c through envmod.BatchedModular2D._upload with the stand-in world; the caller has set the case's environment.
    Returns the record (JSON types only)."""
    import torch
    events, worlds, streams = [], [], []

    class StandInWorld:
        def __init__(self, n_envs, lanes, flags=0, device=None, wide=False, options=None):
            self.n_envs, self.lanes, self.flags, self.device = n_envs, lanes, flags, torch.device("cpu")
            self.k = len(worlds)
            worlds.append({"n_envs": int(n_envs), "lanes": int(lanes), "flags": int(flags), "device": device, "wide": wide,
                           "options": None if options is None else dict(options), "tile_shape": "never reset", "outputs": None})
            events.append("create %d" % self.k)

        def set_terrain(self, terrain):
            assert terrain == "the terrain"
            events.append("terrain %d" % self.k)

        def reset(self, morph, tile_shape=None):
            assert (morph.n_envs, morph.lanes) == (self.n_envs, self.lanes)
            worlds[self.k]["tile_shape"] = tile_shape
            events.append("reset %d" % self.k)

        def set_outputs(self, reward, done, index):
            assert index.dtype == torch.int32 and reward.numel() == done.numel()
            worlds[self.k]["outputs"] = sha(index.numpy(), np.int32)
            events.append("outputs %d" % self.k)

        def close(self):
            events.append("close %d" % self.k)

    def group_streams(device, n):
        streams.append(n)
        return [None] * n

    saved = envmod.BatchedWorld, envmod.group_streams
    envmod.BatchedWorld, envmod.group_streams = StandInWorld, group_streams
    try:
        env = new_env(envmod, c)
        env._terrain = lambda: "the terrain"
        batches, n = batches_of(c)
        for (m, _), b in zip(batches, c["buckets"]):
            assert envmod._uniform(m) == b[2], "case %s: a bucket is not what it says" % c["name"]
        env._upload(batches, n)
    finally:
        envmod.BatchedWorld, envmod.group_streams = saved
    group_of = {wi: g for g, ws in enumerate(env.groups) for wi in ws}
    for wi, (w, idx) in enumerate(env.worlds):
        worlds[wi]["group"] = group_of[wi]
        worlds[wi]["index"] = sha(idx.numpy(), np.int64)
    return {"groups": [list(g) for g in env.groups], "group_streams": streams, "tile_shape_used": env._tile_shape_used,
            "tile_shape_by_lanes": sorted(env._tile_shape_by_lanes.items()), "launch_options": env._launch_options,
            "world_flags": int(env._world_flags), "rebalance_steps": int(env._rebalance_steps),
            "public": [env.merged_launch, env.step_groups, env.use_graph, env.rebalance_every],
            "buffers": [int(env._reward.numel()), int(env._fitness.numel())], "worlds": worlds, "events": events}


def jsonable(rec):
    return json.loads(json.dumps(rec))   # (tuples -> lists, as the recorded file has them)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("checkout", help="root of the checkout whose gym_rem2d_amd is recorded")
    ap.add_argument("-o", "--output", default="launch_plans.json")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.checkout))
    from gym_rem2d_amd import env as envmod
    assert os.path.abspath(envmod.__file__).startswith(os.path.abspath(args.checkout) + os.sep), envmod.__file__
    out = {}
    for c in CASES:
        for v in OVERRIDE_VARS:
            os.environ.pop(v, None)
        os.environ.update(c["env"])
        out[c["name"]] = run_case(envmod, c)
    assert len(out) == len(CASES), "case names must be unique"
    with open(args.output, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(out), args.output))


if __name__ == "__main__":
    main()
