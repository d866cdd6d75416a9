"""The closed loop stated on the host (include/rem2d_control.h), shared by tests/test_control_host.py (oracle alone) and
tests/test_control_gpu.py: what render_model.py is for the renderer.

* ``observe_model``: the observation rows in numpy binary32, from what ``state_forge.snapshot`` reads out of oracle worlds (which
  includes ``w.wod``).  Each arithmetic result is one numpy float32 operation, i.e. separately rounded like the kernel's __fsub_rn.
* ``policy``: the fixed controller of every loop test, a host function of (step, observation rows) in binary64: a per-body sine
  reference, minus a gain times the observed joint angle, plus a term on the touching count, clamped to +-pi/2.  The same numbers
  go to the oracle (``World.set_controller``) and to the GPU (``set_joint_targets``).
* ``OracleLoop``: a lane bucket of oracle worlds with the env bookkeeping of state_forge and the two controller writes.
* ``closed_loop_run``: the oracle's side of the loop protocol, cached: observation after reset and after every step, final state.

Why a joint target needs no change to a step: the controller computes (amp * sin(i_state + phase)) + offset in binary64; with
amp = 0.0 the product is +-0 for every finite argument, so the target is `offset` exactly (test_control_host.py asserts the motor
speed that follows).
"""
import math

import numpy as np

import state_forge as F

OBS_HEAD, OBS_BODY = 8, 6
N_LOOP = 300                      # closed-loop steps of the parity runs
# the policy's constants: chosen so that the oracle ALONE shows the loop to matter (test_control_host.py: >= 90 % of the creatures
# end somewhere else than under their own oscillators)
REF_AMP, REF_RATE, REF_BODY_PHASE = 0.9, 0.21, 0.8
ANGLE_GAIN, TOUCH_GAIN = 0.35, 0.25


def width(max_bodies):
    return OBS_HEAD + OBS_BODY * max_bodies


def observe_model(ctx, snap, max_bodies):
    """float32 [N, 8 + 6 * max_bodies]: row e = creature e of the lane bucket `ctx`, body b = lane ctx.slots[e][b]."""
    f32 = np.float32
    obs = np.zeros((ctx.N, width(max_bodies)), f32)
    for e in range(ctx.N):
        sl = ctx.slots[e]
        row = obs[e]
        for q, f in enumerate(F.BODY_F):
            row[q] = snap[f][e, 0]
        row[6] = f32(np.float64(snap["px"][e, 0]) - np.float64(snap["wod"][e]))
        row[7] = f32(len(sl))
        for b, lane in enumerate(sl[:max_bodies]):
            blk = row[OBS_HEAD + b * OBS_BODY:OBS_HEAD + (b + 1) * OBS_BODY]
            n = int(snap["ccount"][e, lane])
            blk[3] = f32(int((snap["cnpt"][:n, e, lane] > 0).sum()))
            if b == 0:
                continue
            p = int(ctx.parent[e, lane])
            blk[0] = f32(f32(snap["ang"][e, lane] - snap["ang"][e, p]) - f32(0.0))
            blk[1] = f32(snap["w"][e, lane] - snap["w"][e, p])
            blk[2] = f32(int(snap["jlimit"][e, lane]))
            blk[4] = f32(snap["px"][e, lane] - snap["px"][e, 0])
            blk[5] = f32(snap["py"][e, lane] - snap["py"][e, 0])
    return obs


def policy(t, obs, max_bodies):
    """Joint targets float64 [N, max_bodies] for the step that follows observation `obs` (float32 rows), t = steps taken so far."""
    o = np.asarray(obs, dtype=np.float64)
    body = o[:, OBS_HEAD:].reshape(o.shape[0], max_bodies, OBS_BODY)
    b = np.arange(max_bodies, dtype=np.float64)
    ref = REF_AMP * np.sin(REF_RATE * float(t) + REF_BODY_PHASE * b)
    target = ref[None, :] - ANGLE_GAIN * body[:, :, 0] + TOUCH_GAIN * body[:, :, 3]
    return np.clip(target, -math.pi / 2, math.pi / 2)


class OracleLoop:
    """The oracle worlds of one lane bucket (Morphology) under external control."""

    def __init__(self, O, terrain, morph, flags, pop=None):
        self.ctx = F.Ctx(morph, pop)
        self.ot = F.oracle_terrain(O, terrain)
        md = morph.as_dict()
        N = self.ctx.N
        self.worlds = [O.World.from_morph(self.ot, md, e, flags) for e in range(N)]
        for e, w in enumerate(self.worlds):
            assert w.n_bodies == len(self.ctx.slots[e]) and w.n_joints == w.n_bodies - 1
        self.env = dict(reward=np.zeros(N, np.float32), done=np.zeros(N, np.int32), everdone=np.zeros(N, np.int32),
                        fitness=np.zeros(N, np.float64), frozen=np.zeros(N, np.int32), steps=np.zeros(N, np.int32))
        # the controller words the host has to hand back unchanged (set_controller takes all of them): [N][K][amp phase freq offset]
        self.ctl = np.stack([self.ctx.field(f).astype(np.float64) for f in ("amp", "phase", "freq", "offset")], axis=-1)

    def step(self):
        env = self.env
        for e, w in enumerate(self.worlds):
            r, d = w.env_step()
            env["reward"][e], env["done"][e] = r, d
            env["everdone"][e] |= d
            if not env["frozen"][e]:    # evaluate()'s fitness rule, as in state_forge.oracle_run
                if r < -10.0:
                    env["frozen"][e] = 1
                elif r > 100.0:
                    env["fitness"][e], env["frozen"][e] = r + (10000 - env["steps"][e]) / 10000.0, 1
                elif r > 0.0:
                    env["fitness"][e] = r
            env["steps"][e] += 1

    def snapshot(self):
        return F.snapshot(self.ctx, self.worlds, self.env)

    def _write(self, e, b, amp, phase, freq, offset, istate):
        self.ctl[e, self.ctx.slots[e][b]] = (amp, phase, freq, offset)
        self.worlds[e].set_controller(b - 1, float(amp), float(phase), float(freq), float(offset), float(istate))

    def set_targets(self, targets, mask=None):
        """REM2D_CTRL_TARGET: column b -> the joint between body b and its parent (oracle joint b - 1): amp 0, offset target."""
        for e, w in enumerate(self.worlds):
            ist = w.controller_state()
            sl = self.ctx.slots[e]
            for b in range(1, min(len(sl), targets.shape[1])):
                if mask is None or mask[e, b]:
                    _, phase, freq, _ = self.ctl[e, sl[b]]
                    self._write(e, b, 0.0, phase, freq, targets[e, b], ist[b - 1])

    def set_params(self, params, mask=None):
        """REM2D_CTRL_PARAMS: params [N, M, 4] = amp, phase, freq, offset."""
        for e, w in enumerate(self.worlds):
            ist = w.controller_state()
            for b in range(1, min(len(self.ctx.slots[e]), params.shape[1])):
                if mask is None or mask[e, b]:
                    self._write(e, b, *params[e, b], ist[b - 1])

    def root_x(self):
        return np.array([w.bodies()[0, 0] for w in self.worlds], np.float32)


def chain_population(n=12, modules=8):
    """(terrain, [Morphology]) of 8-module chains standing in a row: the fixed-morphology population."""
    from gym_rem2d_amd import make_terrain, synthetic
    return make_terrain(4), [synthetic.chain_population(n, modules, "left")]


_LOOP_POPS = {}


def loop_population(name):
    """(terrain, [Morphology per lane bucket]) of the loop tests: state_forge's populations without the creatures that are a lone
    root module (24 of the 40 L-system creatures of lane bucket 2, 30 of the 117 CPPN creatures): no controller can move those.
    They are observed in test_control_gpu.py's plumbing test, which takes the population as it is."""
    if name == "chain8":
        return chain_population()
    if name not in _LOOP_POPS:
        terrain, morphs = F.population(name)
        kept = []
        for m in morphs:
            jointed = np.flatnonzero((m.arrays["shape"].reshape(m.n_envs, m.lanes) != 0).sum(axis=1) >= 2)
            if len(jointed):
                kept.append(m if len(jointed) == m.n_envs else m.take(jointed))
        _LOOP_POPS[name] = (terrain, kept)
    return _LOOP_POPS[name]


_RUNS = {}


def closed_loop_run(O, pop, flags, n_steps=N_LOOP, params_at=None):
    """The oracle under `policy` for every lane bucket of population `pop` -> list of dict(ctx, max_bodies, obs [n_steps + 1][N, W]
    (after reset, after every step), targets [n_steps][N, M], final (snapshot), caps [n_steps + 1][N, 2] (most pairs / touching
    contacts on a body: who leaves a build's comparison when).  params_at = (step, params function): at that step the controllers
    are set with REM2D_CTRL_PARAMS instead (params function(ctx) -> [N, M, 4]) and run open loop from there."""
    key = (pop, flags, n_steps, params_at and params_at[0])
    if key in _RUNS:
        return _RUNS[key]
    terrain, morphs = loop_population(pop)
    runs = []
    for morph in morphs:
        loop = OracleLoop(O, terrain, morph, flags, pop)
        ctx, M = loop.ctx, morph.lanes
        snap = loop.snapshot()
        run = dict(ctx=ctx, max_bodies=M, obs=[observe_model(ctx, snap, M)], targets=[], caps=[], params=None)

        def caps(s):
            return np.stack([s["ccount"].max(axis=1), ((s["ctouch"] != 0) & F.masks(ctx, s)["cedge"]).sum(axis=0).max(axis=1)], 1)
        run["caps"].append(caps(snap))
        open_loop = False
        for t in range(n_steps):
            if params_at is not None and t == params_at[0]:
                run["params"] = params_at[1](ctx)
                loop.set_params(run["params"])
                open_loop = True
            if not open_loop:
                tg = policy(t, run["obs"][-1], M)
                loop.set_targets(tg)
                run["targets"].append(tg)
            loop.step()
            snap = loop.snapshot()
            for f in F.LANE_FIELDS + F.SLOT_FIELDS:
                assert np.isfinite(snap[f]).all(), "oracle state not finite: %s %s step %d" % (pop, f, t + 1)
            run["obs"].append(observe_model(ctx, snap, M))
            run["caps"].append(caps(snap))
        run["final"] = snap
        run["root_x"] = loop.root_x()
        runs.append(run)
    _RUNS[key] = runs
    return runs


def left_out_first(run, pair_slots=24, solver_slots=6):
    """-> first [N]: index into run["obs"] from which the creature is left out of a comparison with a build of these slots
    (len(obs) = never), bits [N]: the capacity bits the oracle's state justifies."""
    n = len(run["caps"])
    first, bits = np.full(run["ctx"].N, n, np.int32), np.zeros(run["ctx"].N, np.int32)
    for t, c in enumerate(run["caps"]):
        b = np.where(c[:, 0] > pair_slots, F.ERR_PAIR, 0) | np.where(c[:, 1] > solver_slots, F.ERR_SOLVER, 0)
        new = (b != 0) & (first == n)
        first[new], bits[new] = t, b[new]
    return first, bits
