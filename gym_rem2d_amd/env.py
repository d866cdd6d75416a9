"""gym-shaped environments on top of the batched MI355X stepper.

``Modular2D`` keeps the reference env's surface (``gym_rem2D/envs/Modular2DEnv.py:127-173,
565-653``): ``seed(int) -> [seed]``, ``reset(tree=, module_list=) -> None``,
``step(action) -> (0, reward, done, 0)``, attributes ``action_space``, ``observation_space``,
``hardcore``, ``robot.components/joints``, ``tree_morphology``, ``wod``.  It is a batch of one.

``BatchedModular2D`` is the same environment for N creatures at once: ``reset(trees,
module_lists)`` compiles every tree into the SoA layout, groups creatures by lane count
(homogeneous waves) and uploads them; ``step(n)`` advances all of them n steps on the GPU and
returns ``reward[N]`` / ``done[N]`` torch tensors.  ``render()`` draws them on the device (gym_rem2d_amd.render);
the reference's pyglet window (``:655-768``) is out of scope.
"""
import copy
import ctypes as C

import numpy as np
import torch

from . import _lib, control, gymshim, launch_policy, sense
from .compiler import Morphology, build_creature, lanes_for
from .launch_policy import _uniform  # noqa: F401  (its home now; still importable from here)
from .terrain import make_terrain
from .world import BatchedWorld

FPS = 50
WOD_SPEED = 0.04
VIEWPORT_W, VIEWPORT_H, SCALE = 800, 600, 30.0


class ModularRobotBox2D:
    """robot.components / robot.joints containers (Modular2DEnv.py:69-82)."""

    def __init__(self):
        self.components, self.joints = [], []

    def add_components(self, components, joints=None):
        self.components.extend(components)
        if joints is not None:
            self.joints.extend(joints)
        return self


class WallOfDeath:
    def __init__(self, speed):
        self.position = 0.0
        self.speed = speed

    def update(self):
        self.position += self.speed


class Episodes:
    """BatchedModular2D.episodes: the persistent population-order buffers reset_where() writes (include/rem2d_episode.h,
    rem2d_episode_out), all ``[N]`` on the env's device.  ``reward`` float32 / ``done`` bool: every creature's reward / done as the last
    step left them, read before anything was reset.  ``ended`` bool: whom the last call reset.  ``fitness`` float64 / ``steps`` int32:
    evaluate()'s fitness and the length of the creature's LAST ended episode.  ``count`` int32: episodes ended since the upload."""
    FIELDS = ("reward", "done", "ended", "fitness", "steps", "count")

    def __init__(self, n, device):
        z = torch.zeros
        self.reward = z(n, dtype=torch.float32, device=device)
        self.done = z(n, dtype=torch.bool, device=device)
        self.ended = z(n, dtype=torch.bool, device=device)
        self.fitness = z(n, dtype=torch.float64, device=device)
        self.steps = z(n, dtype=torch.int32, device=device)
        self.count = z(n, dtype=torch.int32, device=device)

    def descriptor(self):
        out = _lib.EpisodeOut()
        out.reward, out.done, out.ended = self.reward.data_ptr(), self.done.data_ptr(), self.ended.data_ptr()
        out.fitness, out.steps, out.episodes = self.fitness.data_ptr(), self.steps.data_ptr(), self.count.data_ptr()
        return out


def when_bits(when):
    """The REM2D_WHEN_* bit set of a subset of ("done", "frozen", "steps") (a single name is accepted too)."""
    if isinstance(when, str):
        when = (when,)
    bits = 0
    for name in when or ():
        if name not in _lib.WHEN:
            raise ValueError("when: unknown condition %r (known: %s)" % (name, ", ".join(sorted(_lib.WHEN))))
        bits |= _lib.WHEN[name]
    return bits


class Stream:
    """BatchedModular2D.stream: the record of a streamed evaluation (include/rem2d_stream.h), on the env's device.  Indexed by the
    population's ids, ``[n_total]``: ``fitness`` float64 / ``steps`` int32 / ``err`` int32 (REM2D_ERR_* bits) of a creature's episode,
    written when refill() finds it ended, and ``finished`` bool.  ``occupant`` int32 ``[slots]``: the id of the creature in each slot
    (population-row order of the env), -1 = retired.  ``cursors`` int32, one per lane bucket: pending creatures handed out so far (it
    may run past the bucket's pending count: ``handed_out()`` clamps it)."""

    def __init__(self, n_total, occupant, pending, device):
        z = torch.zeros
        self.fitness = z(n_total, dtype=torch.float64, device=device)
        self.steps = z(n_total, dtype=torch.int32, device=device)
        self.err = z(n_total, dtype=torch.int32, device=device)
        self.finished = z(n_total, dtype=torch.bool, device=device)
        self.occupant = occupant
        self.pending = list(pending)                  # pending creatures per lane bucket (host)
        self.cursors = z(len(self.pending), dtype=torch.int32, device=device)

    def descriptor(self):
        out = _lib.StreamOut()
        out.fitness, out.steps, out.err, out.finished = (self.fitness.data_ptr(), self.steps.data_ptr(), self.err.data_ptr(),
                                                         self.finished.data_ptr())
        return out

    def handed_out(self):
        """Pending creatures handed out so far, per lane bucket (a host read: it waits for the queued calls)."""
        return [min(int(c), n) for c, n in zip(self.cursors.cpu().tolist(), self.pending)]


def stream_slots(counts, lanes, slots):
    """How many of ``slots`` each lane bucket gets (reset_stream): proportional to the buckets' creature counts, the slots left over
    by the whole parts going one by one to the bucket that is furthest below its share (largest remainder; ties to the earlier
    bucket), never more than the bucket has creatures.  Every bucket starts from a floor of ``min(count, 64 // lanes)`` -- one whole
    wavefront of slots -- where ``slots`` covers those floors, else from one slot: fewer slots than buckets raise ValueError."""
    counts = [int(c) for c in counts]
    if any(c <= 0 for c in counts):
        raise ValueError("reset_stream: an empty lane bucket")
    if slots < len(counts):
        raise ValueError("reset_stream: slots = %d is below the number of lane buckets (%d): every bucket needs a slot"
                         % (slots, len(counts)))
    total = sum(counts)
    slots = min(int(slots), total)
    have = [min(c, max(1, 64 // K)) for c, K in zip(counts, lanes)]
    if sum(have) > slots:
        have = [1] * len(counts)
    share = [slots * c / float(total) for c in counts]
    for _ in range(slots - sum(have)):
        k = max((k for k in range(len(counts)) if have[k] < counts[k]), key=lambda k: (share[k] - have[k], -k))
        have[k] += 1
    return have


_GROUP_STREAMS = {}   # device -> the step-group streams of this process


def group_streams(device, n):
    """The n - 1 HIP streams step groups 1 .. n-1 run on (group 0 runs on the caller's stream), shared by every
    BatchedModular2D of the process: HIP maps streams onto a few hardware queues and streams that share a queue serialise,
    so a second env must not bring streams of its own (65 536 CPPN creatures: 24.8 M env-steps/s on the 6th-8th stream
    of a process, 45 M on the first three)."""
    dev = torch.device(device if device is not None else "cuda")
    index = dev.index if dev.index is not None else torch.cuda.current_device()   # (None, "cuda", "cuda:0": ONE pool)
    pool = _GROUP_STREAMS.setdefault(index, [])
    while len(pool) < n - 1:
        pool.append(torch.cuda.Stream(device=device))
    return [None] + pool[:max(0, n - 1)]


class BatchedModular2D:
    MAX_WORLD_LANES = 1 << 22   # rem2d_world_create refuses ~5 M lanes and more (32-bit lane offsets)
    BIG_POPULATION = 131072     # creatures per GPU from which the 128-lane tiles of the velocity kernel pay (round 4: 2 joint
                                # register sets at 4 wavefronts per SIMD, 18.6 active lanes; profiles/r04_sweep_population_shape.txt)
    REBALANCE_EVERY = 50        # env-steps between two re-orderings of a mixed population by current cost (see __init__)
    TRAIN128_MAX = 131072       # creatures per GPU up to which the 128-lane step train is used instead of per-step launches (profiles/
                                # r06_train128.txt; on the round's final build: 131 072: 71.4 vs 71.3 M env-steps/s, 163 840: 76.1 vs 78.6 M,
                                # 196 608: 75.5 vs 82.6 M -- the 4-phase loop and -Os helped the per-step launches more)
    TRAIN128_UNIFORM = False    # uniform populations on the static 128-lane shape keep per-step launches on three step groups: 65 536 8-module
                                # chains 180.7 M against 177.0 M as a train (and 142.5 M as a 64-lane train) -- profiles/r06_train128.txt

    def __init__(self, hardcore=False, flat=False, seed=4, device=None, flags=None, wide=False, options=None, on_handover="raise"):
        # pybox2d's b2World() defaults: continuousPhysics on, sleeping on
        # options: launch options for every world ({name: value}, _lib.OPTIONS -- launch forms, never results), e.g.
        # {"fuse_velpost": 1} = per-step launches instead of the step train.  on_handover: what step() / fitness / errors() do when a
        # step train reported failed hand-overs (rem2d_world_handover_failures): "raise" _lib.HandoverError (nothing computed from
        # such a state is handed out silently), or "flag" = leave it to the caller, who reads errors() & ERR_HANDOVER
        # (evaluate.run_episode: re-evaluates those creatures on per-step launches)
        # wide: the worlds live in librem2d_wide.so (32 pair slots / 12 solver slots per body; evaluate.run_episode re-runs
        # there the creatures that overflowed the default build's slots)
        from . import _lib
        self.wide = wide if wide == "fma" else bool(wide)   # ("fma": the labelled -ffp-contract=fast tolerance mode, not bit-exact)
        self.hardcore, self.flat = hardcore, flat
        self.flags = _lib.FLAG_CONTINUOUS if flags is None else flags
        self.device = device
        self._seed = seed
        self.terrain = None
        self.worlds = []      # list of (BatchedWorld, env index tensor)
        self.n_envs = 0
        self.trees = None
        self.robots = None
        self._reward = self._done = None
        self._policy = self._act_args = None   # set_policy()
        self._context_reset = False            # reset_where() since the last act(): whom it restarted reads zero context (RecurrentPolicy)
        self._episodes = self._episode_args = self._autoreset = None   # episodes / reset_where() / set_autoreset()
        self._stream_rec = self._refill_args = None                    # reset_stream() / refill() / stream
        self._descriptor = None                                        # set_descriptor() / describe() / behaviour
        self.last_episode = None      # evaluate.EpisodeReport of the population in place (None: no episode since its upload)
        over = launch_policy.read_overrides()   # (REM2D_MERGED_LAUNCH, REM2D_STEP_GROUPS, REM2D_GRAPH, REM2D_REBALANCE: read here, once)
        self.merged_launch = over.merged_launch   # False: step every lane bucket on its own stream instead of one merged grid
        self.step_groups = over.step_groups       # 0 = automatic
        # launch shape of the velocity kernel (rem2d_world_set_tile_shape): None = automatic, unless the experiment
        # override REM2D_TILE_SHAPE fixes it (_lib.env_tile_shape).  Up to ~150 000 creatures a step is bound by its chain of stragglers and the
        # 64-lane tiles (4 wavefronts per SIMD) win; beyond that the chip's instruction issue saturates and the 256-lane
        # tiles (2.4x fewer wave-instructions) do: 62.1 vs 58.0 M env-steps/s at 196 608 creatures.
        self.tile_shape = None
        self.groups, self.group_streams = [], []
        self._group_args = None
        self._plan = None             # launch_policy.Plan of the population in place (made by _upload)
        self.use_graph = over.use_graph   # replay every step call as a hipGraph
        # Creature order by current cost: every `rebalance_every` env-steps the creatures that used every position iteration in
        # the last step are moved to the front of their world's order (a stable partition: the static schedule order survives
        # within both classes), so that they share velocity tiles and position blocks -- a tile costs what its most expensive
        # creature costs.  Made on the device by the library itself (launch option `rebalance`, rem2d_rebalance_kernel: one
        # small launch per world every N steps).  -1: automatic (50 for mixed populations: +3.3 % on config 3, +3 % on the
        # 131 072-creature generation against REM2D_FLAG_RETILE, which it replaces as the policy; +0.5 % on config 4; -0.8 % at
        # 1 M creatures), 0: off.  REM2D_REBALANCE overrides (experiments); rebalance() does the same from the host.
        self.rebalance_every = over.rebalance_every
        self.options = dict(options or {})
        if on_handover not in ("raise", "flag"):
            raise ValueError("on_handover must be 'raise' or 'flag'")
        self.on_handover = on_handover

    def seed(self, seed=None):
        self._seed = seed
        self.terrain = None
        return [seed]

    def _terrain(self):
        if self.terrain is None:
            self.terrain = make_terrain(self._seed, hardcore=self.hardcore, flat=self.flat)
        return self.terrain

    # ---- reset from phenotype trees (reference-shaped) ----
    def reset(self, trees, module_lists=None):
        """trees: list of Tree; module_lists: list (or one shared list) of module prototypes.
        Like the reference, each tree is deep-copied so that the env owns controller state."""
        if module_lists is None or (len(module_lists) > 0 and not isinstance(module_lists[0], (list, tuple))):
            module_lists = [module_lists] * len(trees)
        self.module_lists = list(module_lists)   # (render.tree_colors: the reference colours a body by node.type / len(module_list))
        self.trees, self.robots, specs = [], [], []
        for tree, ml in zip(trees, module_lists):
            t = copy.deepcopy(tree)
            spec, comps, joints = build_creature(t.getNodes(), ml)
            self.trees.append(t)
            self.robots.append(ModularRobotBox2D().add_components(comps, joints))
            specs.append(spec)
        self.reset_specs(specs)
        self._bind_views()

    def reset_specs(self, specs):
        groups = {}
        for e, s in enumerate(specs):
            groups.setdefault(lanes_for(s.n_bodies), []).append(e)
        batches = []
        desc = launch_policy.read_overrides().sort_desc   # (REM2D_SORT_DESC)
        for lanes in sorted(groups):
            # creatures of one wave run in lockstep: keep waves homogeneous in joint rounds / size
            # (the most complex first: their wavefronts are the long ones and should be dispatched first)
            idx = sorted(groups[lanes], key=lambda e: (specs[e].period, max(specs[e].rounds, default=-1), specs[e].n_bodies),
                         reverse=desc)
            batches.append((Morphology.from_specs([specs[e] for e in idx], lanes), idx))
        self._upload(batches, len(specs))

    def reset_morphology(self, morph):
        """Fast path: a precompiled SoA batch (one lane count)."""
        self.reset_batches([(morph, list(range(morph.n_envs)))])

    def reset_batches(self, batches, n_envs=None):
        """Precompiled lane-bucket batches [(Morphology, population indices)] (encode.batches_from_compiled, population.compile);
        n_envs: the population's size (None: the batches' total)."""
        self.trees = self.robots = None
        self._upload(batches, sum(m.n_envs for m, _ in batches) if n_envs is None else n_envs)

    def _upload(self, batches, n_envs):
        for w, _ in self.worlds:
            w.close()
        self.worlds = []
        self._world_morph = []   # host-side layout of every world's creatures (compact() re-plans tiles from it)
        self._uploaded = [(m, np.asarray(idx, dtype=np.int64)) for m, idx in batches]   # (evaluate.run_episode's fallback)
        self._compacted = False
        self.last_episode = None
        self._inactive = set()   # worlds compact() found without a single open fitness
        self._group_args = None
        self.n_envs = n_envs
        self.streams = []
        self._obs = None                                       # observe()'s persistent buffer: made (zeroed) on first use after a reset
        self._obs_bodies = max(m.lanes for m, _ in batches)    # default max_bodies of observe(): the largest lane bucket
        self._ctl_keep = None
        self._sense = None                                     # sense_terrain()'s persistent (frac, hit) buffers, made on first use
        self._sense_rays = {}                                  # ray tables on the device, by content
        self._policy = None                                    # set_policy(): the device policy and its persistent buffers
        self._act_args = None
        self._context_reset = False
        self._episodes = None                                  # reset_where()'s harvest buffers: made (zeroed) on first use after a reset
        self._episode_args = None
        self._stream_rec = self._refill_args = None            # (a streamed evaluation ends with the upload that replaces it)
        self._descriptor = None                                # set_descriptor(): period, samples and the behaviour buffer
        # how this population runs -- step groups, tile shape, train or per-step launches, rebalancing, which creatures share a
        # world -- is launch_policy.plan's decision, from the buckets' shapes, this env's settings and the REM2D_* overrides
        plan = self._plan = self._make_plan(batches, n_envs)
        # (the names bench.py, tests and tools read)
        self._tile_shape_used, self._tile_shape_by_lanes, self._launch_options = plan.tile_shape, plan.tile_shape_by_lanes, plan.launch_options
        self._world_flags, self._rebalance_steps = plan.world_flags, plan.rebalance_steps
        self.groups = [[] for _ in range(plan.groups)]
        for piece in plan.pieces:
            morph, idx = self._uploaded[piece.bucket]
            part = morph if len(piece.members) == morph.n_envs else morph.take(piece.members)
            w = self._new_world(part.n_envs, part.lanes)
            w.reset(part, tile_shape=plan.tile_shape_by_lanes.get(part.lanes, plan.tile_shape))
            self.groups[piece.group].append(len(self.worlds))
            self.worlds.append((w, torch.as_tensor(idx[piece.members], dtype=torch.long, device=w.device)))
            self._world_morph.append(part)
        self.groups = [g for g in self.groups if g]
        dev = self.worlds[0][0].device
        # the first group runs on the caller's stream: four streams in all is what the device overlaps well (a fifth costs
        # 5-25 %: 4 groups on 4 new streams 36.7 M, on the caller's + 3 new ones 40.2 M env-steps/s for config 3)
        self.group_streams = group_streams(dev, len(self.groups))
        self._reward = torch.zeros(n_envs, dtype=torch.float32, device=dev)
        self._done = torch.zeros(n_envs, dtype=torch.bool, device=dev)
        self._fitness = torch.zeros(n_envs, dtype=torch.float64, device=dev)
        self._frozen_pop = torch.zeros(n_envs, dtype=torch.int32, device=dev)
        self._steps_pop = torch.zeros(n_envs, dtype=torch.int32, device=dev)
        self._err_pop = torch.zeros(n_envs, dtype=torch.int32, device=dev)
        if len(self.worlds) > 1:
            # the kernels write reward / done straight into these population-order arrays (rem2d_world_set_outputs):
            # step() returns them without a gather per world
            for w, idx in self.worlds:
                w.set_outputs(self._reward, self._done, idx.to(torch.int32))
        elif not np.array_equal(self._uploaded[0][1], np.arange(n_envs)):
            # one world whose creature order is not the population's (reset_specs sorts a lane bucket by schedule): observe() and
            # set_joint_targets() find the population row of a creature through the same index (decided here, on the host array)
            w, idx = self.worlds[0]
            w.set_outputs(self._reward, self._done, idx.to(torch.int32))

    def _make_plan(self, batches, n_envs):
        knobs = launch_policy.Knobs(self.step_groups, self.tile_shape, self.flags, self.options, self.rebalance_every,
                                    self.BIG_POPULATION, self.TRAIN128_MAX, self.TRAIN128_UNIFORM, self.REBALANCE_EVERY,
                                    self.MAX_WORLD_LANES, _lib.MAX_STEP_GROUPS, _lib.MAX_WORLDS_PER_STEP)
        return launch_policy.plan([launch_policy.bucket(m) for m, _ in batches], n_envs, knobs, launch_policy.read_overrides())

    def _world_options(self):
        return self._plan.world_options

    def _new_world(self, n_envs, lanes):
        """A world of this env: its device and build, the plan's flags and options, the terrain."""
        w = BatchedWorld(n_envs, lanes, self._plan.world_flags, self.device, wide=self.wide, options=self._world_options())
        w.set_terrain(self._terrain())
        return w

    def handover_failures(self, clear=False):
        """Failed hand-overs of the step train over all worlds (host-side counters, no synchronisation: what the launches that have
        finished so far reported)."""
        return sum(w.handover_failures(clear) for wi, (w, _) in enumerate(self.worlds) if getattr(w, "h", None))

    def check_handover(self, sync=False):
        """Raise _lib.HandoverError if a step train of this env reported failed hand-overs (unless on_handover == "flag").  sync:
        wait for the queued launches first -- the counters only know what has finished."""
        if self.on_handover != "raise" or not self.worlds:
            return
        if sync:
            torch.cuda.synchronize(self.worlds[0][0].device)
        n = self.handover_failures()
        if n:
            raise _lib.HandoverError(n)

    def _bind_views(self):
        """Let node.component / robot.components read live poses (host read-back; API parity only)."""
        if self.robots is None:
            return
        where = {}
        for w, idx in self.worlds:
            for local, e in enumerate(idx.tolist()):
                where[e] = (w, local)
        for e, robot in enumerate(self.robots):
            w, local = where[e]

            def live(slot, w=w, local=local):
                return (float(w.view("px")[local, slot]), float(w.view("py")[local, slot]),
                        float(w.view("ang")[local, slot]))
            for b in robot.components:
                b._live = live

    # ---- step ----
    def step(self, n_steps=1):
        if not self.groups and len(self.worlds) != 1:   # compact() has retired every world: nothing left to step
            return self._reward, self._done
        self.check_handover()   # (nothing more is queued behind a launch that reported a failed hand-over)
        if len(self.worlds) == 1:
            self.worlds[0][0].step(n_steps)
        elif (self.merged_launch and len(self.groups) <= _lib.MAX_STEP_GROUPS
              and all(len(g) <= _lib.MAX_WORLDS_PER_STEP for g in self.groups)):
            # all lane buckets of a group in one grid per kernel, all groups in ONE ABI call (rem2d_groups_step): fork from
            # the caller's stream, the steps of the groups queued round-robin, join -- or the whole call replayed as a
            # hipGraph (REM2D_GRAPH=1)
            if self._group_args is None:
                arrs = [_lib.world_array(self.worlds[i][0] for i in g) for g in self.groups]
                sg = (_lib.StepGroup * len(self.groups))()
                for k, (g, st) in enumerate(zip(self.groups, self.group_streams)):
                    sg[k].worlds = C.cast(arrs[k], C.POINTER(C.c_void_p))
                    sg[k].n_worlds = len(g)
                    sg[k].stream = None if st is None else st.cuda_stream
                self._group_args = (sg, arrs)
            _lib.check(_lib.lib(self.wide).rem2d_groups_step(self._group_args[0], len(self.groups), int(n_steps),
                                                             self.worlds[self.groups[0][0]][0]._stream(),
                                                             _lib.STEP_GRAPH if self.use_graph else 0), self.wide)
        else:
            # fallback path (REM2D_MERGED_LAUNCH=0, or more lane buckets than one launch takes): one HIP stream per world,
            # created on first use
            cur = torch.cuda.current_stream(self.worlds[0][0].device)
            while len(self.streams) < len(self.worlds):
                self.streams.append(torch.cuda.Stream(device=self.worlds[0][0].device))
            for wi, ((w, _), st) in enumerate(zip(self.worlds, self.streams)):
                if wi in self._inactive:
                    continue
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    w.step(n_steps)
            for st in self.streams:
                cur.wait_stream(st)
        # (no synchronisation: this sees the launches that have finished -- a failure of the call just queued surfaces at the next
        # step(), or at fitness / errors(), which wait first)
        self.check_handover()
        if len(self.worlds) == 1 and not self._compacted:
            w = self.worlds[0][0]
            return w.view("reward"), w.view("done") != 0
        return self._reward, self._done   # written by the step's own kernels (set_outputs in _upload)

    def rebalance(self, pos_iters=60):
        """The host-side form of the `rebalance` launch option (which does the same on the device every N steps): give every
        world a creature order by CURRENT cost through rem2d_world_set_order -- the creatures that used all `pos_iters`
        position iterations in the last step (a joint at its limit pressed against the ground; the same creatures for many
        steps) go to the front, in their static order, the others follow in theirs.  A few small torch kernels per world,
        queued on the caller's stream like the steps; no effect on any result."""
        for wi, (w, _) in enumerate(self.worlds):
            if wi in self._inactive or (w.flags & _lib.FLAG_RETILE) or w.n_envs < 2 * (64 // min(64, w.lanes)):
                continue
            slow = w.view("positers") >= pos_iters
            w.set_order(torch.sort((~slow).to(torch.uint8), stable=True).indices, check=False)   # (a sort's indices)

    def launch_info(self):
        """(tile shape, launch form) of the first step group -- the library's own answer (rem2d_worlds_launch_info: 2 = the step
        train, 1 = velocity tiles and position iterations in one launch per step, 0 = two launches); for tools that name
        kernels, results never depend on it."""
        idx = self.groups[0] if self.groups else list(range(len(self.worlds)))
        arr = _lib.world_array(self.worlds[i][0] for i in idx)
        shape, fused = C.c_int32(), C.c_int32()
        _lib.check(_lib.lib(self.wide).rem2d_worlds_launch_info(arr, len(idx), C.byref(shape), C.byref(fused)), self.wide)
        return shape.value, int(fused.value)

    def _gather(self, name, out):
        if len(self.worlds) == 1 and not self._compacted:
            return self.worlds[0][0].view(name).clone()   # a snapshot, like the multi-world path
        # (creatures compact() has dropped keep the values it stored in `out`; the others are copied by the library's own kernel --
        # torch's index_copy_ here loaded a code object at its first launch, tens of ms inside a caller's first read)
        for wi, (w, _) in enumerate(self.worlds):
            if wi not in self._inactive:
                w.gather(name, out)
        return out.clone()   # (`out` is the persistent population-order buffer compact() writes to: callers get a snapshot)

    # ---- evaluate(): drop the creatures whose fitness is final ----
    def compact(self, min_envs=2048, max_alive=0.5):
        """Between two steps of an evaluate() episode: when at most ``max_alive`` of the creatures of a lane bucket still
        have an open fitness (REM2D_F_FROZEN == 0), the bucket's worlds (one per step group) are replaced by ONE smaller
        world that holds only those -- state moved field by field, rem2d_world_adopt -- so that the wavefronts of the
        finished creatures stop costing anything (REM2D_FLAG_SKIP_FROZEN only stops wavefronts whose creatures have ALL
        finished) and the few survivors of a long episode are stepped by one launch sequence instead of one per step
        group.  Fitness / steps / error bits of the dropped creatures stay readable through the population-order
        properties.  Buckets with fewer than ``min_envs`` creatures are left alone.  Returns the number of creatures
        still being stepped."""
        if self._stream_rec is not None:
            raise ValueError("compact: this env streams its population through a fixed window of slots (reset_stream): a finished "
                             "creature's slot is refilled by refill(), there is nothing to compact")
        by_lanes = {}
        for wi, (w, idx) in enumerate(self.worlds):
            if wi not in self._inactive:
                by_lanes.setdefault(w.lanes, []).append(wi)
        alive_total = 0
        changed = False
        for lanes, wis in sorted(by_lanes.items()):
            keeps = [torch.nonzero(self.worlds[wi][0].view("frozen") == 0, as_tuple=False).flatten() for wi in wis]
            n_keep = sum(int(k.numel()) for k in keeps)
            n_now = sum(self.worlds[wi][0].n_envs for wi in wis)
            alive_total += n_keep
            if n_now < min_envs or n_keep > max_alive * n_now:
                continue
            changed = True
            for wi in wis:   # what the population-order properties report for the creatures that leave
                w, idx = self.worlds[wi]
                self._fitness.index_copy_(0, idx, w.view("fitness"))
                self._frozen_pop.index_copy_(0, idx, w.view("frozen"))
                self._steps_pop.index_copy_(0, idx, w.view("steps"))
                self._err_pop.index_copy_(0, idx, w.view("err"))
                self._reward.index_copy_(0, idx, w.view("reward"))
                self._done.index_copy_(0, idx, w.view("done") != 0)
            if n_keep == 0:   # nobody left: the worlds stay as they are and are not launched any more
                self._inactive.update(wis)
                continue
            part = Morphology.concat([self._world_morph[wi].take(k.cpu().numpy()) for wi, k in zip(wis, keeps) if k.numel()])
            nw = self._new_world(n_keep, lanes)
            for name in _lib.FIELDS:
                dst = nw.view(name)
                dim = 1 if dst.dim() == 3 else 0
                dst.copy_(torch.cat([self.worlds[wi][0].view(name).index_select(dim, k) for wi, k in zip(wis, keeps)
                                     if k.numel()], dim=dim))
            nw.adopt(part, tile_shape=self._plan.tile_shape)
            new_idx = torch.cat([self.worlds[wi][1][k] for wi, k in zip(wis, keeps) if k.numel()])
            nw.set_outputs(self._reward, self._done, new_idx.to(torch.int32))
            torch.cuda.synchronize(nw.device)   # the old arenas must outlive the copies
            for wi in wis[1:]:   # (the entries stay so that world indices do not move; the arenas go)
                self._inactive.add(wi)
                self.worlds[wi][0].release()
            self.worlds[wis[0]][0].release()
            self.worlds[wis[0]] = (nw, new_idx)
            self._world_morph[wis[0]] = part
        if changed:
            self._compacted = True
            groups = [[i for i in g if i not in self._inactive] for g in self.groups]
            groups = [g for g in groups if g]
            active = [i for g in groups for i in g]
            if sum(self.worlds[i][0].n_envs for i in active) < 16384 and len(active) <= _lib.MAX_WORLDS_PER_STEP:
                groups = [active] if active else []   # too few creatures for step groups to pay: one launch sequence
            self.groups = groups
            self.group_streams = self.group_streams[:max(1, len(groups))]   # (the first is the caller's stream: None)
            self._group_args = None
            self._act_args = None   # (act() masks the rows no live world holds any more)
            self._episode_args = None
        return alive_total

    @property
    def fitness(self):
        """evaluate()'s running fitness (REM2D_main.py:362-377), float64 [N]."""
        self.check_handover(sync=True)
        return self._gather("fitness", self._fitness)

    @property
    def frozen(self):
        return self._gather("frozen", self._frozen_pop)

    @property
    def steps(self):
        """env steps taken since reset, int32 [N]."""
        return self._gather("steps", self._steps_pop)

    def errors(self):
        """REM2D_ERR_* bits per creature, int32 [N] (the one read that never raises HandoverError: it is how a caller finds the
        creatures concerned)."""
        return self._gather("err", self._err_pop)

    # ---- closed loop: what the creatures sense, what the caller sets on their joints (include/rem2d_control.h) ----
    def _control_worlds(self):
        """The worlds still being stepped (the population index each of them carries was installed by _upload / compact)."""
        return [w for wi, (w, _) in enumerate(self.worlds) if wi not in self._inactive and getattr(w, "h", None)]

    @property
    def max_bodies(self):
        """observe()'s default ``max_bodies``: the lanes of the population's largest lane bucket."""
        return self._obs_bodies

    def observe(self, max_bodies=None, out=None):
        """What every creature senses now: float32 ``[N, 8 + 6 * max_bodies]`` on the device, rows in population order, columns as
        ``control.layout(max_bodies)`` names them (root pose and velocity, distance to the wall of death, body count; per body in
        ``robot.components`` order: joint angle, joint speed, limit state, touching contacts, position relative to the root).
        One kernel of the library for the whole population, queued on the current stream like step(); nothing synchronises.
        ``max_bodies``: default the population's largest lane bucket; bodies beyond it are dropped, missing ones read 0.
        ``out``: a contiguous float32 tensor of that shape to write into; without it the env's persistent buffer is returned (zeroed
        at reset, overwritten by the next call: clone what must last).  Rows of creatures that compact() has retired are not
        written any more: they keep their last written observation."""
        M = self._obs_bodies if max_bodies is None else int(max_bodies)
        if out is None:
            if self._obs is None or self._obs.shape[1] != control.width(M):
                self._obs = torch.zeros((self.n_envs, control.width(M)), dtype=torch.float32, device=self.worlds[0][0].device)
            out = self._obs
        worlds = self._control_worlds()
        if worlds:
            control.observe(worlds, M, out)
        return out

    def set_joint_targets(self, targets, mask=None):
        """Closed-loop joint targets for the steps that follow: ``targets`` ``[N, M]`` (float32 or float64, population order), column
        b the target angle (radians) of the joint between body b and its parent, column 0 ignored; ``mask`` ``[N, M]``, false =
        leave that joint as it is.  The joint's controller becomes amp = 0, offset = target, so the step's own PID drives the motor
        towards it (motorSpeed = (target - jointAngle) * 1.9); its phase, frequency and i_state stay.  Values are written as given:
        keep them finite and inside the joint limits (+-pi/2).  Queued on the current stream; with ``targets`` (and ``mask``) on the
        env's device nothing synchronises -- a host array is accepted too, at the price of a blocking upload.

        A creature that overflows the default build's contact slots (errors() & ERR_CAPACITY) cannot be replayed from reset in the
        wide build under external actions, as evaluate.run_episode does for open-loop creatures: read errors(), or construct the env
        with wide=True."""
        self._control(control.CTRL_TARGET, targets, mask)

    def set_controllers(self, params, mask=None):
        """Oscillator parameters for the steps that follow: ``params`` ``[N, M, 4]`` = (amp, phase, freq, offset) of the joint between
        body b and its parent (column 0 ignored), ``mask`` as in set_joint_targets.  The running i_state is never written: a changed
        frequency bends the phase from where it is.  The capacity note of set_joint_targets holds here too."""
        self._control(control.CTRL_PARAMS, params, mask)

    def _control(self, mode, values, mask):
        values = torch.as_tensor(values)
        if values.shape[0] != self.n_envs:
            raise ValueError("expected one row per creature (%d), got %d" % (self.n_envs, values.shape[0]))
        worlds = self._control_worlds()
        if worlds:
            self._ctl_keep = control.control(worlds, mode, values, mask)   # (the tensors the queued kernel reads)

    def _ray_table(self, rays):
        """The ray table on the device: uploaded once, then found again by its bytes."""
        rays = sense.check_rays(sense.bipedal_rays() if rays is None else
                                (rays.detach().cpu().numpy() if isinstance(rays, torch.Tensor) else rays))
        key = rays.tobytes()
        dev = self._sense_rays.get(key)
        if dev is None:
            if len(self._sense_rays) >= 16:      # (a caller that makes a new table per call must not grow this without bound)
                self._sense_rays.clear()
            dev = self._sense_rays[key] = torch.from_numpy(rays.copy()).to(self.worlds[0][0].device)
        return dev

    def sense_terrain(self, rays=None, out=None, hits=False):
        """How far the ground is along rays cast from every creature's root body: float32 ``[N, R]`` on the device, rows in
        population order, column r the fraction of ray r at which it first meets the track's edges or hardcore boxes, 1.0 where it
        meets nothing.  ``rays``: float64 ``[R, 2]`` offsets from the root in the world frame (they do not turn with the root), R
        up to 64; default ``sense.bipedal_rays()``, BipedalWalker's 10-ray fan of length ``sense.LIDAR_RANGE``.  A table is
        uploaded once and found again by its content (passing one blocks for the upload the first time).  ``hits=True`` returns
        ``(frac, hit)``, hit int32 ``[N, R]``: the static proxy met -- hardcore boxes first, then edge i as ``n_polys + i`` -- or
        -1.  One kernel of the library for the whole population, queued on the current stream like step() and observe().
        ``out``: a contiguous float32 ``[N, R]`` tensor to write the fractions into; without it the env's persistent buffer is
        returned (1.0 / -1 at first use, overwritten by the next call: clone what must last).  Rows of creatures that compact() has
        retired are not written any more: they keep their last value."""
        dev_rays = self._ray_table(rays)
        R = int(dev_rays.shape[0])
        dev = self.worlds[0][0].device
        if self._sense is None or self._sense[0].shape[1] != R:
            self._sense = (torch.ones((self.n_envs, R), dtype=torch.float32, device=dev),
                           torch.full((self.n_envs, R), sense.NO_HIT, dtype=torch.int32, device=dev))
        frac = self._sense[0] if out is None else out
        hit = self._sense[1] if hits else None
        worlds = self._control_worlds()
        if worlds:
            sense.sense(worlds, dev_rays, frac, hit)
        return (frac, hit) if hits else frac

    # ---- device policies: the controllers live on the device as data (include/rem2d_policy.h) ----
    def set_policy(self, policy, normalizer=None, accumulate=True):
        """Attach a ``policy.MLPPolicy`` to the population in place (after reset; a new upload drops it), or None to detach it.  The
        policy needs one weight set per creature, or an ``index`` with one entry per creature, and at most 64 bodies' worth of
        columns; it is moved to the env's device.  The buffers act() works in -- observation rows, ray fractions, targets, validity
        bytes -- are allocated here, once.  step(), observe(), sense_terrain() and set_joint_targets() are not affected.

        A ``policy.RecurrentPolicy`` also gets its context words here: ``policy_memory``, float32 ``[N, context]`` in population
        order, zeroed -- attaching a policy again zeroes them again.  act() carries them from step to step and reads zeros for a
        creature that reset_where() has just restarted.  Streaming under a recurrent policy is not built: a slot's next creature
        would inherit its predecessor's context, so with a streamed evaluation in place this raises ValueError.

        A ``policy.ModularPolicy`` -- one controller per body, messages along the tree; one weight set may drive creatures of
        different trees -- gets its messages here, ``policy_memory`` float32 ``[N, max_bodies, messages]``, zeroed, and the
        topology table of the creatures in place (``policy_topology``, as ``topology(policy.max_bodies)`` makes it); a new upload
        drops both with the policy, and attaching the policy again makes them again.  act() then is rem2d_worlds_act_modular, under
        the reset rules of a recurrent policy.  With a ``normalizer`` or a streamed evaluation this raises ValueError: neither is
        built for modular policies.

        ``normalizer``: a ``policy.ObsNormalizer`` of the policy's ``max_bodies`` and rays on the env's device whose blocks cover the
        creatures (``n_blocks * group_size >= n_envs``; creature r belongs to block ``r // group_size``): act() then stages every
        row through the normaliser's tables as they stand (rem2d_worlds_act_normed) and, with ``accumulate``, first adds the rows
        it has just observed to the normaliser's sums -- one launch more; the tables move at the normaliser's next ``freeze()``,
        never by themselves.  Without a normaliser nothing changes."""
        from .policy import ModularPolicy, ObsNormalizer, RecurrentPolicy
        self._act_args = None
        self._context_reset = False
        if policy is None:
            if normalizer is not None:
                raise ValueError("set_policy: a normalizer needs a policy")
            self._policy = None
            return
        if not self.worlds:
            raise ValueError("set_policy: no population in place (reset first)")
        recurrent = isinstance(policy, RecurrentPolicy)
        if recurrent and self._stream_rec is not None:
            raise ValueError("set_policy: a RecurrentPolicy cannot be attached to a streamed evaluation (reset_stream): refill() "
                             "would hand a slot's context to the next creature -- streaming under recurrent policies is not built")
        modular = isinstance(policy, ModularPolicy)
        if modular and normalizer is not None:
            raise ValueError("set_policy: a ModularPolicy takes no normalizer: observation normalisation of per-body rows is not built")
        if modular and self._stream_rec is not None:
            raise ValueError("set_policy: a ModularPolicy cannot be attached to a streamed evaluation (reset_stream): refill() would "
                             "change a slot's tree under the topology table -- streaming under modular policies is not built")
        have = policy.n_sets if policy.index is None else int(policy.index.shape[0])
        if have != self.n_envs:
            raise ValueError("set_policy: the policy has %d %s for %d creatures"
                             % (have, "weight sets" if policy.index is None else "index entries", self.n_envs))
        dev = self.worlds[0][0].device
        policy = policy.to(dev)
        N, M, R = self.n_envs, policy.max_bodies, policy.n_rays
        if normalizer is not None:
            if not isinstance(normalizer, ObsNormalizer):
                raise ValueError("set_policy: normalizer must be a policy.ObsNormalizer")
            normalizer._fits("set_policy", policy, N)
        self._policy = dict(
            normalizer=normalizer, accumulate=bool(accumulate) and normalizer is not None,
            policy=policy, rays=self._ray_table(policy.rays) if R else None,
            obs=torch.zeros((N, control.width(M)), dtype=torch.float32, device=dev),
            frac=torch.ones((N, R), dtype=torch.float32, device=dev) if R else None,
            targets=torch.zeros((N, M), dtype=torch.float64, device=dev),
            valid=torch.zeros((N, M), dtype=torch.uint8, device=dev),
            memory=policy.new_memory(N) if recurrent or modular else None,
            topo=self.topology(M) if modular else None)

    @property
    def policy(self):
        return None if self._policy is None else self._policy["policy"]

    def topology(self, max_bodies=None, out=None):
        """The creatures' trees in body order: int32 ``[N, max_bodies, 2]`` on the device, rows in population order, body b the b-th
        live lane exactly as observe() counts them.  Word 0 is the BODY index of body b's parent -- -1 for the root, for a body whose
        parent has no column below ``max_bodies`` and for the slots beyond the creature's count --, word 1 the body's shape word
        (non-zero: the slot is live; ``compiler`` SHAPE_BOX / SHAPE_CIRCLE).  One kernel of the library for the whole population
        (rem2d_worlds_topology), queued on the current stream; nothing synchronises.  ``out``: a contiguous int32 tensor of that
        shape to write into; without it a new one (-1 / 0 in the rows of creatures that compact() has retired).  The table changes
        only when the creatures do: a reset_where() restarts the same trees."""
        M = self._obs_bodies if max_bodies is None else int(max_bodies)
        if not 1 <= M <= control.MAX_BODIES:
            raise ValueError("topology: max_bodies must be 1..%d, not %r" % (control.MAX_BODIES, max_bodies))
        if not self.worlds:
            raise ValueError("topology: no population in place (reset first)")
        dev = self.worlds[0][0].device
        if out is None:
            out = torch.zeros((self.n_envs, M, 2), dtype=torch.int32, device=dev)
            out[:, :, 0] = -1
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or tuple(out.shape) != (self.n_envs, M, 2)
              or not out.is_contiguous() or out.device != dev):
            raise ValueError("topology: out must be a contiguous torch.int32 [%d, %d, 2] tensor on %s" % (self.n_envs, M, dev))
        worlds = self._control_worlds()
        if worlds:
            w0 = worlds[0]
            t = _lib.Topology()
            t.max_bodies, t.reserved, t.out, t.out_rows, t.stream = M, 0, out.data_ptr(), self.n_envs, w0._stream()
            _lib.check(w0.L.rem2d_worlds_topology(_lib.world_array(worlds), len(worlds), C.byref(t)), w0.wide)
        return out

    @property
    def policy_topology(self):
        """The topology table of the attached ``policy.ModularPolicy``: int32 ``[N, max_bodies, 2]``, made by set_policy(); None
        without one."""
        return None if self._policy is None else self._policy.get("topo")

    @property
    def policy_memory(self):
        """The context words of the attached ``policy.RecurrentPolicy``: float32 ``[N, context]`` on the device, population order,
        read and rewritten in place by every act() (clone what must last); None without one.  Under a ``policy.ModularPolicy``: the
        bodies' messages, float32 ``[N, max_bodies, messages]``."""
        return None if self._policy is None else self._policy["memory"]

    def act(self):
        """One control step by the attached policy: every creature is observed (and its rays cast), the policy's forward pass turns
        the rows into joint targets, and the finite ones are written to the joints as set_joint_targets would -- one library call
        (rem2d_worlds_act), four launches queued on the current stream, nothing synchronises.  Returns the persistent ``(targets
        float64 [N, max_bodies], valid uint8 [N, max_bodies])`` buffers the call writes (clone what must last); ``valid`` 0 = the
        target is not finite and that joint was left as it is.  After compact(), rows no live world holds are masked out of the
        forward pass and keep their last values.

        With a normaliser attached (set_policy) the call is rem2d_worlds_act_normed: the same launches, the forward pass staging
        its rows through the normaliser's tables, and one launch more where the rows are also added to its sums; the compacted row
        mask and a recurrent policy's reset mask mean what they mean without one.

        Under a ``policy.RecurrentPolicy`` the call is rem2d_worlds_act_recurrent -- as many launches -- which also carries
        ``policy_memory`` forward.  The first act() after a reset_where() (under set_autoreset: every act()) hands that call's
        ``episodes.ended`` to the kernel as its reset mask: a creature that has just restarted reads zero context, everybody else
        their own; no extra launch, nothing synchronises."""
        P = self._policy
        if P is None:
            raise ValueError("act: no policy attached (set_policy first)")
        if self._act_args is None:
            worlds = self._control_worlds()
            mask = None
            if self._compacted:
                mask = torch.zeros(self.n_envs, dtype=torch.uint8, device=P["obs"].device)
                for wi, (w, idx) in enumerate(self.worlds):
                    if wi not in self._inactive and getattr(w, "h", None):
                        mask[idx] = 1
            if P.get("topo") is not None:
                desc = P["policy"].descriptor(P["obs"], P["frac"], P["targets"], P["valid"], P.get("topo"), P["memory"], None, mask)
            elif P["memory"] is None:
                desc = P["policy"].descriptor(P["obs"], P["frac"], P["targets"], P["valid"], mask)
            else:
                desc = P["policy"].descriptor(P["obs"], P["frac"], P["targets"], P["valid"], P["memory"], None, mask)
            self._act_args = (worlds, _lib.world_array(worlds) if worlds else None, desc, mask)
        worlds, arr, desc, _ = self._act_args
        if worlds:
            w0 = worlds[0]
            rays = None if P["rays"] is None else P["rays"].data_ptr()
            if P.get("topo") is not None:   # (the stream and the reset mask are this one call's, as below)
                desc.stream = w0._stream()
                desc.reset = self._episodes.ended.data_ptr() if self._context_reset else None
                self._context_reset = False
                try:
                    _lib.check(w0.L.rem2d_worlds_act_modular(arr, len(worlds), C.byref(desc), rays), w0.wide)
                finally:
                    desc.reset = None
            elif P["normalizer"] is not None:
                self._act_normed(P, worlds, arr, desc, rays)
            elif P["memory"] is None:
                _lib.check(w0.L.rem2d_worlds_act(arr, len(worlds), C.byref(desc), rays, w0._stream()), w0.wide)
            else:   # (the reset mask is this one call's: the cached descriptor points at it now and at nothing afterwards)
                desc.reset = self._episodes.ended.data_ptr() if self._context_reset else None
                self._context_reset = False
                try:
                    _lib.check(w0.L.rem2d_worlds_act_recurrent(arr, len(worlds), C.byref(desc), rays, w0._stream()), w0.wide)
                finally:
                    desc.reset = None
        return P["targets"], P["valid"]

    def _act_normed(self, P, worlds, arr, desc, rays):
        """act() under a normaliser: the cached policy descriptor (a recurrent one: its ``p``, the context members travel in the
        normaliser's descriptor) and the normaliser's, on the worlds' stream"""
        norm, w0 = P["normalizer"], worlds[0]
        most = norm._offer("act", self.n_envs) if P["accumulate"] else 0
        n = norm.descriptor()
        p = desc
        if P["memory"] is not None:
            p = desc.p
            n.context, n.memory = desc.context, desc.memory
            n.reset = self._episodes.ended.data_ptr() if self._context_reset else None
            self._context_reset = False
        n.stream = w0._stream()
        _lib.check(w0.L.rem2d_worlds_act_normed(arr, len(worlds), C.byref(n), C.byref(p), rays, int(P["accumulate"])), w0.wide)
        norm.offered += most

    def step_policy(self, n_steps=1):
        """n_steps x (act(), step(1)), queued without any synchronisation: the closed loop with the controller on the device.
        Returns what step() returns.  With set_autoreset() in force every step is followed by reset_where(when, max_steps), and the
        return value is ``(episodes.reward, episodes.done)`` of the last step: the terminal step's values on the rows that ended in
        it, not the zeros their reset left in the arena."""
        out = self._reward, self._done
        auto = self._autoreset
        for _ in range(int(n_steps)):
            self.act()
            out = self.step(1)
            if auto is not None:
                self.reset_where(when=auto[0], max_steps=auto[1])
                out = self._episodes.reward, self._episodes.done
        return out

    # ---- behaviour descriptors: where a creature went, sampled over its episode (include/rem2d_novelty.h) ----
    def set_descriptor(self, period, samples=None):
        """Give the population in place (after reset; a new upload drops it) a behaviour descriptor: the root position sampled
        ``samples`` = K times (1 .. 16), every ``period`` steps, in ``behaviour``, float32 ``[N, 2 * samples]`` on the device, rows
        in population order, allocated here, once, zeroed.  ``set_descriptor(None)`` detaches it.  Nothing records by itself:
        ``describe()`` does, and ``evaluate.run_behaviour_episode`` calls it at the right steps.  step(), step_policy(), act()
        and reset_where() are not affected.

        Auto-reset and streaming are out of scope with a descriptor: a finished episode's row would be overwritten by the next
        episode's before anyone reads it.  While ``set_autoreset`` is in force or a streamed evaluation is in place this raises
        ValueError (and so does ``describe()``)."""
        if period is None:
            self._descriptor = None
            return
        if not self.worlds:
            raise ValueError("set_descriptor: no population in place (reset first)")
        if self._autoreset is not None or self._stream_rec is not None:
            raise ValueError("set_descriptor: descriptors are not recorded under auto-reset or streaming: a finished episode's row "
                             "would be overwritten before anyone reads it (set_autoreset(None) / upload the population with reset*)")
        if samples is None or not 1 <= int(samples) <= _lib.NOVELTY_MAX_SAMPLES:
            raise ValueError("set_descriptor: samples must be 1 .. %d, not %r" % (_lib.NOVELTY_MAX_SAMPLES, samples))
        if int(period) < 1 or int(period) > 2 ** 31 - 1:
            raise ValueError("set_descriptor: period must be 1 .. 2^31 - 1 steps, not %r" % (period,))
        self._descriptor = (int(period), int(samples),
                            torch.zeros((self.n_envs, 2 * int(samples)), dtype=torch.float32, device=self.worlds[0][0].device))

    @property
    def behaviour(self):
        """The descriptor buffer of set_descriptor(), float32 ``[N, 2 * samples]`` (clone what must last), or None."""
        return None if self._descriptor is None else self._descriptor[2]

    def describe(self):
        """Record where every creature is now: a creature whose episode is still running (not frozen) writes its root position
        to every slot k of its ``behaviour`` row with ``(k + 1) * period >=`` its step count; a creature whose episode is over
        writes nothing, so its row keeps what it held when it ended.  Called once after a reset and then every ``period`` steps,
        slot k holds the position at step ``(k + 1) * period``, or the last one recorded before the episode ended.  One library call
        for all lane buckets and step groups (rem2d_worlds_describe), queued on the current stream like observe(); nothing
        synchronises.  Returns ``behaviour``."""
        if self._descriptor is None:
            raise ValueError("describe: no descriptor set (set_descriptor first)")
        if self._autoreset is not None or self._stream_rec is not None:
            raise ValueError("describe: descriptors are not recorded under auto-reset or streaming")
        period, samples, out = self._descriptor
        worlds = self._control_worlds()
        if worlds:
            from . import novelty
            novelty.describe(worlds, period, samples, out)
        return out

    # ---- episode boundaries: a creature starts again the moment it ends (include/rem2d_episode.h) ----
    @property
    def episodes(self):
        """The ``Episodes`` record of the population in place: made (all zero) on first use after a reset, written by reset_where()."""
        if self._episodes is None:
            if not self.worlds:
                raise ValueError("episodes: no population in place (reset first)")
            self._episodes = Episodes(self.n_envs, self.worlds[0][0].device)
        return self._episodes

    def reset_where(self, mask=None, when=(), max_steps=None):
        """Begin a new episode for SOME creatures, in place, between two steps: those whose ``mask`` entry is set (bool / uint8
        ``[N]`` on the env's device, population order; None = everyone) AND for whom one of the ``when`` conditions holds -- a subset
        of ``("done", "frozen", "steps")``: the last step ended at the wall of death, evaluate()'s loop has ended, the episode has
        run ``max_steps`` steps; empty = no condition.  One of the two must be given: everyone at once is reset*()'s job.  A selected
        creature is rebuilt from its morphology exactly as a reset builds it and continues bit for bit like the same creature in a
        freshly reset env; nobody else is touched.  Its joints are back under its own oscillators until the next act() /
        set_joint_targets(): joint targets live in the controller words a reset rewrites.

        One library call for all lane buckets and step groups (rem2d_worlds_reset_where), queued on the current stream; nothing
        synchronises.  Before anything is reset, ``episodes`` receives every creature's reward / done of the last step, and for the
        creatures that end, the fitness and length of the episode; their ``count`` goes up by one.  Returns ``episodes.ended``, the
        persistent bool ``[N]`` buffer of whom this call reset (clone what must last).

        Needs the device morphology of the last reset: after compact() the worlds hold adopted creatures without one, and the call
        raises ValueError."""
        if not self.worlds:
            raise ValueError("reset_where: no population in place (reset first)")
        bits = when_bits(when)
        steps = 0 if max_steps is None else int(max_steps)
        if bits & _lib.WHEN["steps"] and steps <= 0:
            raise ValueError("reset_where: when 'steps' needs max_steps > 0")
        if mask is None and bits == 0:
            raise ValueError("reset_where: neither a mask nor a condition: that would reset everyone, which is reset()'s job")
        if mask is not None:
            dev = self.worlds[0][0].device
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError("reset_where: mask must be a torch.bool or torch.uint8 tensor")
            if tuple(mask.shape) != (self.n_envs,) or not mask.is_contiguous():
                raise ValueError("reset_where: mask must be a contiguous tensor of one entry per creature [%d], not %s"
                                 % (self.n_envs, list(mask.shape)))
            if mask.device != dev:
                raise ValueError("reset_where: mask must be on %s, not %s" % (dev, mask.device))
        if self._episode_args is None:
            if self._compacted or any(getattr(w, "_morph_dev", None) is None for w in self._control_worlds()):
                raise ValueError("reset_where: compact() has moved creatures into adopted worlds, which keep no device morphology to "
                                 "reset from -- upload the population again (reset*) instead of compact() where episodes restart")
            worlds = self._control_worlds()
            morphs = (_lib.Morph * len(worlds))()
            for m, w in zip(morphs, worlds):
                for k in _lib.MORPH_FIELDS:
                    setattr(m, k, w._morph_dev[k].data_ptr())
            self._episode_args = (worlds, _lib.world_array(worlds), morphs, self.episodes.descriptor())
        worlds, arr, morphs, out = self._episode_args
        self._episode_mask = mask   # (the tensor the queued kernel reads)
        w0 = worlds[0]
        _lib.check(w0.L.rem2d_worlds_reset_where(arr, morphs, len(worlds), None if mask is None else mask.data_ptr(), bits, steps,
                                                 C.byref(out), self.n_envs, w0._stream()), w0.wide)
        self._context_reset = True   # (the next act() of a RecurrentPolicy reads `ended` as its reset mask; then never again)
        return self._episodes.ended

    def set_autoreset(self, when=("done", "steps"), max_steps=4800):
        """Let step_policy() follow every step with ``reset_where(when=when, max_steps=max_steps)``: a creature whose episode ends
        starts the next one at once, on the device, and ``episodes`` collects the results.  ``when``: a non-empty subset of
        ("done", "frozen", "steps"); ``max_steps``: the episode length for "steps" (gym's TimeLimit).  ``set_autoreset(None)``
        switches it off.  step(), observe() and act() are not affected."""
        if when is None:
            self._autoreset = None
            return
        bits = when_bits(when)
        if bits == 0:
            raise ValueError("set_autoreset: `when` must name at least one condition (None switches auto-reset off)")
        steps = 0 if max_steps is None else int(max_steps)
        if bits & _lib.WHEN["steps"] and steps <= 0:
            raise ValueError("set_autoreset: when 'steps' needs max_steps > 0")
        self._autoreset = ((when,) if isinstance(when, str) else tuple(when), steps)

    # ---- streaming evaluation: a population of any size through a fixed window of slots (include/rem2d_stream.h) ----
    def reset_stream(self, batches, n_total, slots):
        """Begin a streamed evaluation of a whole population: ``batches`` as reset_batches takes them -- [(Morphology, ids)] per lane
        bucket, ``ids`` the creatures' indices in [0, n_total) -- of which only ``slots`` creatures are in an arena at any time.  Per
        lane bucket the first ``slots_k`` creatures (``stream_slots``) are uploaded as reset_batches uploads them and the others
        become the bucket's feed on the device, from which refill() takes the next one whenever a slot's creature has finished.  The
        env then holds ``slots`` creatures (``n_envs``, reward / done, observe() rows: the slots), and ``stream`` holds the results
        by id.  A slot takes creatures of its own lane count only.

        The launch plan is launch_policy.plan's as always.  The worlds must be on a flexible tile shape (1, 2, 3: its tile table does
        not depend on the creatures in it); a plan on the static shapes 0 or 4 (fixed-morphology populations beyond 2 048 blocks
        per step group, REM2D_TILE_SHAPE) raises ValueError -- set ``env.tile_shape = 3`` there."""
        batches = [(m, np.asarray(idx, dtype=np.int64)) for m, idx in batches]
        n_total = int(n_total)
        if sum(m.n_envs for m, _ in batches) != n_total or any(len(idx) != m.n_envs for m, idx in batches):
            raise ValueError("reset_stream: the batches must hold every creature of the population (%d) once" % n_total)
        if len({m.lanes for m, _ in batches}) != len(batches):
            raise ValueError("reset_stream: one batch per lane count")
        per = stream_slots([m.n_envs for m, _ in batches], [m.lanes for m, _ in batches], int(slots))
        n_slots = sum(per)
        first, rows, at = [], [], 0
        for (m, idx), k in zip(batches, per):
            first.append((m if k == m.n_envs else m.take(np.arange(k)), np.arange(at, at + k)))
            rows.append(np.arange(at, at + k))
            at += k
        plan = self._make_plan(first, n_slots)
        for m, _ in first:
            shape = plan.tile_shape_by_lanes.get(m.lanes, plan.eff_tile_shape)
            if shape in (0, 4):
                raise ValueError("reset_stream: the launch plan puts the %d-lane bucket on the static tile shape %d, whose tile table "
                                 "is planned from the joints of the creatures in it -- its slots cannot take other creatures (set "
                                 "env.tile_shape = 3, or drop the REM2D_TILE_SHAPE override)" % (m.lanes, shape))
        self.trees = self.robots = None
        self._upload(first, n_slots)
        dev = self.worlds[0][0].device
        occupant = torch.full((n_slots,), -1, dtype=torch.int32, device=dev)
        feeds = {}
        rec = Stream(n_total, occupant, [m.n_envs - k for (m, _), k in zip(batches, per)], dev)
        for b, ((m, idx), k, r) in enumerate(zip(batches, per, rows)):
            occupant[torch.as_tensor(r, dtype=torch.long, device=dev)] = torch.as_tensor(idx[:k], dtype=torch.int32, device=dev)
            feed = _lib.Feed()
            feed.count, feed.lanes = m.n_envs - k, m.lanes
            feed.cursor = rec.cursors[b:b + 1].data_ptr()
            keep = None
            if feed.count:
                rest = m.take(np.arange(k, m.n_envs))
                keep = {f: torch.from_numpy(np.ascontiguousarray(rest.arrays[f])).to(dev) for f in _lib.MORPH_FIELDS}
                keep["id"] = torch.as_tensor(idx[k:], dtype=torch.int32, device=dev)
                for f in _lib.MORPH_FIELDS:
                    setattr(feed.M, f, keep[f].data_ptr())
                feed.id = keep["id"].data_ptr()
            feeds[m.lanes] = (feed, keep)   # (the tensors the queued kernels read)
        rec.feeds = feeds
        self._stream_rec = rec

    @property
    def stream(self):
        """The ``Stream`` record of the streamed evaluation in place (reset_stream); dropped by every upload."""
        if self._stream_rec is None:
            raise ValueError("stream: no streamed evaluation in place (reset_stream first)")
        return self._stream_rec

    def refill(self, when=("frozen", "steps"), max_steps=None):
        """Between two steps of a streamed evaluation: every slot whose creature's episode has ended -- one of the ``when``
        conditions holds, as in reset_where -- has that creature's fitness / steps / error bits written to ``stream`` under its id,
        and takes the next pending creature of its lane bucket, rebuilt exactly as a reset builds it; with nobody pending the slot is
        retired (frozen, ``occupant`` -1).  One library call for all worlds (rem2d_worlds_refill), queued on the current stream;
        nothing synchronises.  Returns ``stream``.  An attached policy is left alone: a row keeps its controller set."""
        rec = self._stream_rec
        if rec is None:
            raise ValueError("refill: no streamed evaluation in place (reset_stream first)")
        if self._policy is not None and self._policy.get("topo") is not None:
            raise ValueError("refill: a ModularPolicy is attached: a slot's next creature would have another tree than the topology "
                             "table holds -- streaming under modular policies is not built")
        if self._policy is not None and self._policy["memory"] is not None:
            raise ValueError("refill: a RecurrentPolicy is attached: a slot's next creature would inherit its predecessor's context "
                             "-- streaming under recurrent policies is not built")
        bits = when_bits(when)
        steps = 0 if max_steps is None else int(max_steps)
        if bits == 0:
            raise ValueError("refill: `when` must name at least one condition")
        if bits & _lib.WHEN["steps"] and steps <= 0:
            raise ValueError("refill: when 'steps' needs max_steps > 0")
        if self._refill_args is None:
            worlds = self._control_worlds()
            morphs = (_lib.Morph * len(worlds))()
            feeds = (_lib.Feed * len(worlds))()
            for i, w in enumerate(worlds):
                for k in _lib.MORPH_FIELDS:
                    setattr(morphs[i], k, w._morph_dev[k].data_ptr())
                feeds[i] = rec.feeds[w.lanes][0]
            self._refill_args = (worlds, _lib.world_array(worlds), morphs, feeds, rec.descriptor())
        worlds, arr, morphs, feeds, out = self._refill_args
        w0 = worlds[0]
        _lib.check(w0.L.rem2d_worlds_refill(arr, morphs, len(worlds), feeds, rec.occupant.data_ptr(), bits, steps, C.byref(out),
                                            rec.fitness.numel(), self.n_envs, w0._stream()), w0.wide)
        return rec

    def render(self, creatures=None, mode='rgb_array', **kw):
        """Frames of the creatures as they stand now: uint8 [n, H, W, 3] on the device (gym's rgb_array layout, one image per
        creature), drawn by the library's renderer (render.render_frames, which takes the keyword arguments: width, height,
        camera, fill, line).  ``creatures``: population indices, default all.  Only ``mode='rgb_array'`` exists here."""
        if mode != 'rgb_array':
            raise NotImplementedError("BatchedModular2D.render: only mode='rgb_array'")
        from .render import render_frames
        return render_frames(self, range(self.n_envs) if creatures is None else creatures, **kw)

    def close(self):
        for w, _ in self.worlds:
            w.close()
        self.worlds = []


class Modular2D(gymshim.Env):
    """Single-creature facade with the reference's call signatures."""
    metadata = {'render.modes': ['human', 'rgb_array'], 'video.frames_per_second': FPS}
    hardcore = False

    DEFAULT_MAX_BODIES = 32

    def __init__(self, random_seed=None, device=None, closed_loop=False, max_bodies=DEFAULT_MAX_BODIES, wide=False, lidar=False,
                 policy=None):
        """closed_loop=False: the reference's surface -- step(action) ignores the action and returns observation 0.
        closed_loop=True: ``observation_space`` is the ``8 + 6 * max_bodies`` floats of BatchedModular2D.observe (columns:
        control.layout(max_bodies)), ``action_space`` ``max_bodies`` joint target angles within +-pi/2 (column b: the joint between
        ``robot.components[b]`` and its parent; column 0 is ignored); reset() returns the first observation and step(action)
        applies the action (None: leave the joints as they are) and returns the next one as a numpy array.  A creature that
        overflows the default build's contact slots cannot be replayed in the wide build under external actions: read
        ``env._batch.errors()``, or construct the env with wide=True.
        lidar=True (closed loop only): BipedalWalker's 10 lidar fractions (BatchedModular2D.sense_terrain with sense.bipedal_rays())
        follow the ``8 + 6 * max_bodies`` words; ``observation_space`` is that much wider.  The reference advertises them
        (24 = 14 + 10 floats) and never fills them.
        policy (closed loop only): a ``policy.MLPPolicy`` with one weight set and ``max_bodies`` columns; step(None) then acts by it
        (BatchedModular2D.act) instead of leaving the joints as they are.  An explicit action still wins.  A
        ``policy.RecurrentPolicy`` works the same way: its context words are the batch env's ``policy_memory``, zero after reset()."""
        self._device = device
        self._policy = policy
        if policy is not None:
            if not closed_loop:
                raise ValueError("policy= needs closed_loop=True")
            if policy.max_bodies != int(max_bodies) or (policy.n_sets if policy.index is None else int(policy.index.shape[0])) != 1:
                raise ValueError("policy= must have one weight set (or a one-entry index) and max_bodies = %d columns" % int(max_bodies))
        self.closed_loop, self.max_bodies, self._wide = bool(closed_loop), int(max_bodies), wide
        self.lidar = bool(lidar)
        if self.lidar and not self.closed_loop:
            raise ValueError("lidar=True needs closed_loop=True (the open-loop env returns observation 0, like the reference)")
        self._n_lidar = len(sense.bipedal_rays()) if self.lidar else 0
        self.seed(random_seed)
        self.viewer = None
        self.tree_morphology = None
        self.robot = None
        self.world = None
        self.wod = None
        self.game_over = False
        high = np.array([np.inf] * 24)
        self.action_space = gymshim.Box(np.array([-1, -1, -1, -1]), np.array([1, 1, 1, 1]), dtype=np.float32)
        self.observation_space = gymshim.Box(-high, high, dtype=np.float32)
        if self.closed_loop:
            if not 1 <= self.max_bodies <= control.MAX_BODIES:
                raise ValueError("max_bodies must be 1..%d" % control.MAX_BODIES)
            high = np.full(control.width(self.max_bodies) + self._n_lidar, np.inf)
            self.observation_space = gymshim.Box(-high, high, dtype=np.float32)
            lim = np.full(self.max_bodies, np.pi / 2)
            self.action_space = gymshim.Box(-lim, lim, dtype=np.float32)
        self._batch = None

    def seed(self, seed=None):
        self.np_random, seed = gymshim.np_random(seed)
        self._seed_value = seed
        return [seed]

    def reset(self, tree=None, module_list=None):
        self.wod = WallOfDeath(WOD_SPEED)
        self.game_over = False
        if self._batch is not None:
            self._batch.close()
        self._batch = None
        self.tree_morphology = None
        self.robot = ModularRobotBox2D()
        if tree is None:
            return
        self._batch = BatchedModular2D(hardcore=self.hardcore, seed=self._seed_value, device=self._device, wide=self._wide)
        self._batch.reset([tree], [module_list])
        self.tree_morphology = self._batch.trees[0]
        self.robot = self._batch.robots[0]
        self.world = self._batch.worlds[0][0]
        # the reference counts the expressed controllers in every step (Modular2DEnv.py:617-630); the tree cannot change
        # between resets, so count once
        self._n_ctrl = sum(1 for n in self.tree_morphology.nodes
                           if n.controller is not None and n.expressed and n.component is not None)
        # reward / done of every step land in pinned, device-mapped host memory, written by the step's own kernels
        # (rem2d_world_set_outputs): step() needs no copy kernel and no device -> host memcpy, only the stream's completion
        self._pin_reward = torch.zeros(1, dtype=torch.float32).pin_memory()
        self._pin_done = torch.zeros(1, dtype=torch.bool).pin_memory()
        self._pin_index = torch.zeros(1, dtype=torch.int32, device=self.world.device)
        self.world.set_outputs(self._pin_reward, self._pin_done, self._pin_index)
        if self._policy is not None:
            self._batch.set_policy(self._policy)
        if self.closed_loop:
            self._obs_dev = torch.zeros((1, control.width(self.max_bodies)), dtype=torch.float32, device=self.world.device)
            self._pin_obs = torch.zeros(control.width(self.max_bodies) + self._n_lidar, dtype=torch.float32).pin_memory()
            return self._observe()
        return

    def _observe(self):
        """The creature's observation row as a numpy array (closed loop): observe kernel, copy to pinned memory, one wait."""
        self._batch.observe(self.max_bodies, out=self._obs_dev)
        W = self._obs_dev.shape[1]
        self._pin_obs[:W].copy_(self._obs_dev[0], non_blocking=True)
        if self.lidar:
            self._pin_obs[W:].copy_(self._batch.sense_terrain()[0], non_blocking=True)
        torch.cuda.current_stream(self.world.device).synchronize()
        return self._pin_obs.numpy().copy()

    def step(self, action):
        if self.wod:
            self.wod.update()
        if self.tree_morphology is None:
            raise Exception("no tree_morphology")
        assert self._n_ctrl - 1 == len(self.robot.joints)
        if self.closed_loop and action is not None:
            a = np.asarray(action, dtype=np.float64).reshape(1, -1)
            if a.shape[1] != self.max_bodies:
                raise ValueError("action must have %d entries (max_bodies), got %d" % (self.max_bodies, a.shape[1]))
            self._batch.set_joint_targets(torch.from_numpy(a))
        elif self._policy is not None:
            self._batch.act()
        self.world.step(1)                      # one creature: straight to the C ABI, no bucket / group bookkeeping
        obs = self._observe() if self.closed_loop else 0   # (waits for the stream like the line below)
        torch.cuda.current_stream(self.world.device).synchronize()
        r, d = float(self._pin_reward[0]), bool(self._pin_done[0])   # (host reads of the mapped buffer the kernels wrote)
        return obs, (r if not d else -100), (True if d else 0), 0

    def render(self, mode='human'):
        """The reference paints into a pyglet window (Modular2DEnv.py:655-738; pyglet is not a dependency here).
        ``mode='rgb_array'`` returns the same picture -- terrain, module boxes / circles, joint anchors, wall of death,
        camera following the root -- as an ``[H, W, 3] uint8`` array drawn with matplotlib (Agg) from a state dump of
        the current step; ``mode='human'`` is refused (no window system on this path)."""
        if mode != 'rgb_array':
            raise NotImplementedError("only mode='rgb_array' is available (no pyglet window on the accelerated path); "
                                      "statedump.record_episode + tools/render_dump.py write whole runs")
        if self._batch is None:
            raise Exception("no tree_morphology")
        import matplotlib
        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
        from matplotlib.patches import Circle, Polygon
        from . import statedump
        head = statedump.header(self._batch, [0])
        fr = statedump.frame(self._batch, [0], 0)
        prims = statedump.frame_to_draw_list(head, fr)[0]
        cx = fr["creatures"][0]["pose"][0][0]
        fig, ax = plt.subplots(figsize=(VIEWPORT_W / 100.0, VIEWPORT_H / 100.0), dpi=100)
        ax.plot(head["terrain"]["x"], head["terrain"]["y"], color="#356635", lw=1.5)
        for box in head["terrain"]["boxes"]:
            ax.add_patch(Polygon(box, closed=True, color="#444444"))
        for p in prims:
            if p[0] == "polygon":
                ax.add_patch(Polygon(p[1], closed=True, facecolor="#7fa6d9", edgecolor="#1f3f66"))
            elif p[0] == "circle":
                ax.add_patch(Circle(p[1], p[2], facecolor="#d9a67f", edgecolor="#66401f"))
            else:
                ax.plot([p[1][0]], [p[1][1]], "k.", ms=3)
        ax.axvline(fr["creatures"][0]["wall_of_death"], color="red", lw=1)
        half = VIEWPORT_W / SCALE / 2
        ax.set_xlim(cx - half, cx + half)
        ax.set_ylim(0, VIEWPORT_H / SCALE)
        ax.set_aspect("equal")
        ax.axis("off")
        fig.subplots_adjust(0, 0, 1, 1)
        fig.canvas.draw()
        img = np.asarray(fig.canvas.buffer_rgba())[..., :3].copy()
        plt.close(fig)
        return img

    def close(self):
        if self._batch is not None:
            self._batch.close()
            self._batch = None
