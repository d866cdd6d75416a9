"""Launch policy of BatchedModular2D: how a population is run, decided from its shape alone.

``plan(buckets, n_envs, knobs, overrides)`` is a pure function -- numbers in, one ``Plan`` out; no device, no library call -- of
the population's lane buckets (``Bucket``), the env's settings and class constants as they stand (``Knobs``) and the ``REM2D_*``
experiment overrides of the environment (``read_overrides()``, the one place where those variables are read).
``BatchedModular2D._upload`` builds the worlds the plan lists; ``compact()`` reads the same plan.  No result depends on anything
decided here.  ``tests/test_launch_policy.py`` pins the plans to ``tests/golden/launch_plans.json``, recorded from the ``_upload``
this module was cut out of (``tools/record_launch_plans.py``).
"""
import os
from collections import namedtuple

import numpy as np

from . import _lib

Bucket = namedtuple("Bucket", "n_envs lanes uniform")   # one lane bucket of the population, in upload order

# What _upload reads from the env: its public attributes (step_groups, tile_shape, flags, options, rebalance_every), the class
# constants of BatchedModular2D (where their measurements are) and the library's limits (_lib.MAX_STEP_GROUPS / MAX_WORLDS_PER_STEP)
Knobs = namedtuple("Knobs", "step_groups tile_shape flags options rebalance_every big_population train128_max train128_uniform "
                            "rebalance_default max_world_lanes max_step_groups max_worlds_per_step")

# The REM2D_* launch overrides.  The first four are the initial values of the env's attributes of those names, read when it is
# constructed (the planner takes the attributes, through Knobs); sort_desc is read by reset_specs, the rest by every _upload.
Overrides = namedtuple("Overrides", "merged_launch step_groups use_graph rebalance_every sort_desc "
                                    "tile_shape options tile_shape_by_lanes retile group_cut")

Piece = namedtuple("Piece", "bucket group members")   # one world: creatures `members` (int64 indices into the bucket) of lane bucket `bucket`

# groups: step groups asked for (those that get no world are dropped); tile_shape: the shape chosen (None: left to the override
# / the library), eff_tile_shape: the one in effect; launch_options: what the policy adds to the env's options, world_options:
# what every world is created with; train: the population runs as a step train; pieces: the worlds, in creation order
Plan = namedtuple("Plan", "groups tile_shape eff_tile_shape tile_shape_by_lanes world_flags launch_options world_options "
                          "rebalance_steps train pieces")


def _uniform(m):
    """Every creature of the batch has the same tree and solver schedule (fixed-morphology population)."""
    n, K = m.n_envs, m.lanes
    return all(bool((m.arrays[k].reshape(n, K) == m.arrays[k][:K]).all()) for k in ("shape", "parent", "jround"))


def bucket(m):
    return Bucket(m.n_envs, m.lanes, _uniform(m))


def read_overrides():
    """The REM2D_* launch overrides as the environment has them now (experiments: bench.py, tools/)."""
    env = os.environ
    # (a tile shape per lane bucket, "lanes:shape,...", host layer only -- e.g. the light buckets on 128-lane tiles beside the
    # 16-lane bucket on 64-lane ones in ONE launch: the launch takes the kernel of the largest shape)
    by_lanes = {}
    for item in env.get("REM2D_TILE_SHAPE_BY_LANES", "").split(","):
        if ":" in item:
            by_lanes[int(item.split(":")[0])] = int(item.split(":")[1])
    return Overrides(
        merged_launch=env.get("REM2D_MERGED_LAUNCH", "1") != "0",   # 0: step every lane bucket on its own stream instead of one merged grid
        step_groups=int(env.get("REM2D_STEP_GROUPS", "0")),         # 0 = automatic
        use_graph=env.get("REM2D_GRAPH", "0") == "1",               # replay every step call as a hipGraph
        rebalance_every=int(env.get("REM2D_REBALANCE", "-1")),      # -1 = automatic, 0 = off (see BatchedModular2D.__init__)
        sort_desc=env.get("REM2D_SORT_DESC", "1") != "0",
        tile_shape=_lib.env_tile_shape(),
        options=_lib.env_options(),
        tile_shape_by_lanes=by_lanes,
        # REM2D_FLAG_RETILE (the position kernel deals the creatures anew in every step, in arrival order) was round 3's policy
        # for >= 98 304 creatures; the stable re-ordering every 50 steps does better there and also pays at 65 536
        # (profiles/r04_lane_fill_experiments.txt), so the flag is an experiment override now (REM2D_RETILE=1)
        retile=env.get("REM2D_RETILE") == "1",
        group_cut=env.get("REM2D_GROUP_SPLIT") == "cut")


def plan(buckets, n_envs, knobs, over):
    # Step groups: a step is a chain of four launches, each as long as its slowest wavefront; independent parts of the
    # population on their own streams let one part's tail run under another part's kernels.  (Creatures are
    # independent, so any split is legal.)  What counts is the number of 64-lane blocks and how long a step is: below
    # ~3 000 blocks the chip is not full anyway (4 096 4-module chains: 23.0 M env-steps/s with one group, 20.3 M with
    # two); mixed or wide-creature populations, whose steps take more than a millisecond, gain up to four groups
    # (65 536 L-system creatures, 7 790 blocks: 26 / 36 / 39 / 40 M with 1 / 2 / 3 / 4; CPPN creatures on the
    # hardcore terrain 38.7 / 43.2 / 44.3 M with 2 / 3 / 4); small uniform creatures, whose steps are short, three
    # (65 536 8-module chains, 8 192 blocks: 121 / 160 / 171 / 135 M with 1 / 2 / 3 / 4).  Never more than four streams
    # in all, the caller's included (see env.group_streams).
    groups = knobs.step_groups
    blocks = sum(b.n_envs * b.lanes for b in buckets) / 64.0
    if groups <= 0:
        long_steps = len(buckets) > 1 or max(b.lanes for b in buckets) >= 16
        if long_steps:
            groups = 4 if blocks >= 512 else 1   # (8 192 / 16 384 / 24 576 L-system creatures: +13 / +11 / +15 % over one)
        else:
            groups = 3 if blocks >= 6144 else (2 if blocks >= 3072 else 1)
    uniform = all(b.uniform for b in buckets)
    # Tile shape of the velocity kernel: 64-lane tiles up to ~130 000 creatures, 128-lane tiles beyond (see
    # BatchedModular2D.__init__).  Fixed-morphology populations (every creature the same tree: the north-star's "8-module
    # creatures") are the exception: all creatures of a tile need the same slots per iteration, so a bigger tile costs no more per
    # iteration and halves the wavefronts -- 128-lane tiles: 170 M instead of 136 M env-steps/s for 65 536 8-module
    # chains -- once the 64-lane tiles of a step group would no longer fit the chip at once.
    shape = knobs.tile_shape
    if shape is None and over.tile_shape is None:
        shape = 1 if n_envs >= knobs.big_population else 3
        if shape == 3 and blocks / groups > 2048 and uniform:
            shape = 4   # (128-lane tiles with the static phase -> set map: nothing to rotate in a uniform population)
    # The step train (the library's default launch form for 64-lane tiles, REM2D_OPT_FUSE_VELPOST = 2: all steps of a call in
    # one launch, block-steps handed from workgroup to workgroup) is ONE in-order train: it wants the whole population in one
    # group (config 3: 64.8 M env-steps/s with one group, 59 M with two, 39 M with four -- profiles/r05_step_train.txt).
    # Round 6: the 128-lane tile shapes have a train of their own (rem2d_step_train128_kernel: an item = a tile's two blocks).  It
    # wins while a step is bound by the chain of its launches and loses once the chip's instruction issue saturates: shape 1
    # up to TRAIN128_MAX creatures (beyond: per-step launches on four step groups, as before); shape 4 (uniform populations) --
    # see TRAIN128_UNIFORM.
    opts = dict(over.options, **knobs.options)
    eff_shape = shape if shape is not None else over.tile_shape
    launch_options = {}
    if "fuse_velpost" not in opts and ((eff_shape == 1 and n_envs > knobs.train128_max) or (eff_shape == 4 and not knobs.train128_uniform)):
        launch_options["fuse_velpost"] = 1   # (per-step launches; no result depends on it)
        opts["fuse_velpost"] = 1
    train = eff_shape in (3, 1, 4) and not over.retile and \
        opts.get("fuse_velpost", 2) == 2 and opts.get("pipeline", 3) == 3 and opts.get("debug", 0) == 0
    if train and knobs.step_groups <= 0:
        groups = 1      # ... unless its lane buckets, cut into worlds of <= MAX_WORLD_LANES lanes, are more than one launch takes

        def worlds_per_group(g):
            return sum(-(-(-(-b.n_envs // g)) // max(1, knobs.max_world_lanes // b.lanes)) for b in buckets)
        while groups < knobs.max_step_groups and worlds_per_group(groups) > knobs.max_worlds_per_step:
            groups += 1
    world_flags = (knobs.flags | _lib.FLAG_RETILE) if over.retile else (knobs.flags & ~_lib.FLAG_RETILE)
    every = knobs.rebalance_every
    if every < 0:
        every = knobs.rebalance_default if (n_envs >= 4096 and not uniform) else 0
    rebalance_steps = 0 if over.retile else every
    world_options = dict(launch_options, **knobs.options)
    if rebalance_steps > 0:
        world_options.setdefault("rebalance", rebalance_steps)
    pieces = []
    for k, b in enumerate(buckets):
        # which creatures go to which group: wavefront-sized runs of the (schedule-sorted) batch are dealt round-robin,
        # so that every group gets the same mix of simple and complex creatures and the groups reach the join at the
        # end of a step call together (contiguous parts, REM2D_GROUP_SPLIT=cut: 40.2 instead of 40.6 M on config 3)
        if b.n_envs < 4 * groups:
            members = [np.arange(b.n_envs)]
        elif not over.group_cut:
            run = max(1, 64 // b.lanes)
            which = (np.arange(b.n_envs) // run) % groups
            members = [np.nonzero(which == g)[0] for g in range(groups)]
        else:
            cuts = [b.n_envs * g // groups for g in range(groups + 1)]
            members = [np.arange(cuts[g], cuts[g + 1]) for g in range(groups)]
        per = max(1, knobs.max_world_lanes // b.lanes)   # one world addresses its lanes with 32-bit offsets: <= MAX_WORLD_LANES
        for g, mem in enumerate(members):
            for lo in range(0, len(mem), per):
                pieces.append(Piece(k, g, mem[lo:lo + per]))
    return Plan(groups, shape, eff_shape, over.tile_shape_by_lanes, world_flags, launch_options, world_options or None,
                rebalance_steps, train, tuple(pieces))
