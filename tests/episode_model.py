"""Episode boundaries stated on the oracle alone (include/rem2d_episode.h), shared by tests/test_episodes_host.py and
tests/test_episodes_gpu.py: what control_model.py is for observe / control and policy_model.py for the device policies.

``EpisodeModel`` holds one ``oracle.World`` per creature of a loop population (control_model.OracleLoop per lane bucket).  After a
step, ``reset_where`` evaluates the selection rule of rem2d_worlds_reset_where on the oracle's own done / frozen / step count,

    selected = (mask is None or mask[e]) and (when == () or one of the `when` conditions holds),

records the harvest (reward / done of every creature; ended, and fitness / steps / count of the creatures that end) and replaces an
ended creature's world by ``World.from_morph(...)``: a b2World built again, which is what a reset is.  Its env words start over and
its controller words are the morphology's again.  The policy form (``policy=True``) sets, before every step, the joint targets of
policy_model.forward_model on the model's own state, as policy_model.policy_loop_run does.

Capacity: the model also notes, step by step, the most pairs / touching contacts on a body of every creature (``caps``), so that a
test can apply state_forge's left-out rule.  On the L-system loop population nobody comes near the default build's 24 / 6 slots in
the runs used here (tests/test_episodes_host.py asserts it), so every creature is compared everywhere.
"""
import numpy as np

import control_model as M
import policy_model as PM
import range_model as R
import state_forge as F

CONT = 1
WHEN = ("done", "frozen", "steps")
N_OPEN = 320                # open-loop run with when = ("done",): everyone ends at least once, most end twice
N_TIMED, TIMED_STEPS = 130, 60   # when = ("steps",), max_steps 60: two whole episodes and 10 steps of a third
N_POLICY = 200              # the policy form's run


def selected(env, when, max_steps, mask=None):
    """bool [N]: the selection rule on the env words of a lane bucket (control_model.OracleLoop.env)"""
    assert all(w in WHEN for w in when)
    cond = np.ones(len(env["done"]), bool) if not when else np.zeros(len(env["done"]), bool)
    if "done" in when:
        cond |= env["done"] != 0
    if "frozen" in when:
        cond |= env["frozen"] != 0
    if "steps" in when:
        assert max_steps > 0
        cond |= env["steps"] >= max_steps
    assert mask is not None or when, "neither a mask nor a condition"
    return cond if mask is None else cond & (np.asarray(mask) != 0)


class EpisodeModel:
    def __init__(self, O, pop, flags=CONT, policy=False):
        self.O, self.pop, self.flags, self.policy = O, pop, flags, policy
        self.terrain, self.morphs = M.loop_population(pop)
        self.loops = [M.OracleLoop(O, self.terrain, m, flags, pop) for m in self.morphs]
        self.md = [m.as_dict() for m in self.morphs]
        self.ctl0 = [loop.ctl.copy() for loop in self.loops]
        self.n = [loop.ctx.N for loop in self.loops]
        z = lambda dt: [np.zeros(n, dt) for n in self.n]
        self.reward, self.done, self.ended = z(np.float32), z(bool), z(bool)
        self.fitness, self.steps, self.count = z(np.float64), z(np.int32), z(np.int32)
        self.caps = z(np.int32), z(np.int32)          # most pairs / touching contacts on a body so far, per creature
        if policy:
            self.T, self.rays = R.Terrain.of(self.terrain), R.bipedal_rays()
            self.weights = [PM.loop_weights(loop.ctx.N, loop.ctx.K) for loop in self.loops]

    def _act(self):
        for loop, W in zip(self.loops, self.weights):
            snap = loop.snapshot()
            obs = M.observe_model(loop.ctx, snap, PM.LOOP_BODIES)
            frac = R.cast(self.T, snap["px"][:, 0], snap["py"][:, 0], self.rays)[0]
            tg, valid = PM.forward_model(PM.input_rows(obs, frac), *W)
            loop.set_targets(tg, mask=valid)

    def _note_caps(self):
        for k, loop in enumerate(self.loops):
            for e, w in enumerate(loop.worlds):
                for b in range(w.n_bodies):
                    ci = w.contacts(b)[0]
                    if len(ci):
                        self.caps[0][k][e] = max(self.caps[0][k][e], len(ci))
                        self.caps[1][k][e] = max(self.caps[1][k][e], int((ci[:, 3] != 0).sum()))

    def step(self, n=1):
        for _ in range(n):
            if self.policy:
                self._act()
            for loop in self.loops:
                loop.step()
            self._note_caps()

    def reset_where(self, masks=None, when=(), max_steps=0):
        """-> [ended bool [N] per bucket]; masks: None or one array (or None) per bucket"""
        for k, loop in enumerate(self.loops):
            env = loop.env
            sel = selected(env, when, max_steps, None if masks is None else masks[k])
            self.reward[k], self.done[k], self.ended[k] = env["reward"].copy(), env["done"] != 0, sel
            for e in np.flatnonzero(sel):
                self.fitness[k][e], self.steps[k][e] = env["fitness"][e], env["steps"][e]
                self.count[k][e] += 1
                loop.worlds[e] = self.O.World.from_morph(loop.ot, self.md[k], int(e), self.flags)
                for f in ("reward", "done", "everdone", "fitness", "frozen", "steps"):
                    env[f][e] = 0
                loop.ctl[e] = self.ctl0[k][e]
        return [e.copy() for e in self.ended]

    def snapshots(self):
        return [loop.snapshot() for loop in self.loops]

    def over_capacity(self, pair_slots=24, solver_slots=6):
        """[bool [N] per bucket]: creatures the oracle has shown beyond a build's slots at some step (state_forge's left-out rule)"""
        return [(p > pair_slots) | (t > solver_slots) for p, t in zip(*self.caps)]


_RUNS = {}


def run(O, pop, n_steps, when, max_steps=0, masks=None, policy=False, flags=CONT):
    """n_steps x (step, reset_where(masks, when, max_steps)) from reset, cached -> dict(ctxs, ended [n_steps][bucket] bool [N],
    fitness / steps [n_steps][bucket] (the harvest buffers after that step's call), reward / done likewise, count [bucket], final
    [bucket] snapshots, over [bucket] (over_capacity), model)."""
    key = (pop, n_steps, tuple(when), max_steps, None if masks is None else tuple(np.asarray(m).tobytes() for m in masks), policy, flags)
    if key in _RUNS:
        return _RUNS[key]
    model = EpisodeModel(O, pop, flags, policy)
    out = dict(ctxs=[loop.ctx for loop in model.loops], ended=[], fitness=[], steps=[], reward=[], done=[], model=model)
    for _ in range(n_steps):
        model.step()
        out["ended"].append(model.reset_where(masks, when, max_steps))
        for f in ("fitness", "steps", "reward", "done"):
            out[f].append([a.copy() for a in getattr(model, f)])
    out["count"] = [c.copy() for c in model.count]
    out["final"] = model.snapshots()
    out["over"] = model.over_capacity()
    _RUNS[key] = out
    return out


def episode_lengths(r):
    """[per bucket: list per creature of (end step (1-based), steps, fitness) of every ended episode] of a run"""
    out = []
    for k, ctx in enumerate(r["ctxs"]):
        per = [[] for _ in range(ctx.N)]
        for t, ended in enumerate(r["ended"]):
            for e in np.flatnonzero(ended[k]):
                per[e].append((t + 1, int(r["steps"][t][k][e]), float(r["fitness"][t][k][e])))
        out.append(per)
    return out
