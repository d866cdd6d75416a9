"""Step arguments and joint parameters the trajectories never use, shared by the host half (tests/test_step_forge_host.py,
oracle alone) and the GPU half (tests/test_step_forge_gpu.py).

Every other parity test steps with world.Step(1/50, 180, 60) on joints limited to exactly +-pi/2.  A case here is
(population, joint-parameter variant, dt schedule): the variant overwrites lower / upper / torque / amp / offset of the
Morphology BEFORE reset, so that the reset kernel and oracle.World.from_morph read the same binary32 values; the schedule is a
list of (steps, dt, velocity iterations, position iterations), one rem2d_world_step_ex call each, and the oracle's whole
visible state (state_forge.snapshot) is recorded after every step; the GPU half compares after every call.  Values are
computed in binary64 and rounded once to binary32.

Populations: the first 20 creatures of each L-system lane bucket 2 / 4 / 8 / 16 (state_forge.population("lsystem"), rough terrain
seed 4: 80 creatures) and the first 20 two-body creatures ("pairs").  Schedules of the `const` kind are 15 single-step calls and
4 calls of 5 steps (35 steps: both the per-step launches and the step train's hand-over see every dt); `alternating` is 18
calls of 1 / 2 / 3 steps (36 steps) over ten time steps with dtRatio 0 (first step), 0.5, 4, 0.25, 6.67, 0.3, 2, 0.125; `budget_mix`
is tests/test_cpu_twin.py's sequence (25 x 1/50 at 180 / 60, 10 x 1/60 at 8 / 3, 15 x 1/50 at 30 / 0).  `const10+kick30` adds
state_forge's kick30 injection before calls 3 and 10 (single-step calls: the clamp shows as a 2 m step).

What the cases reach is tabulated in tests/test_step_forge_host.py (`python tests/step_forge.py` prints it).
"""
import collections

import numpy as np

import state_forge as F
from state_forge import (ENV_FIELDS, LANE_FIELDS, LEFT_OUT_CAP, SLOT_FIELDS, Ctx, masks, oracle_terrain,  # noqa: F401
                         population, snapshot)

PER_BUCKET = 20
LIM_INACTIVE, LIM_AT_LOWER, LIM_AT_UPPER, LIM_EQUAL = 0, 1, 2, 3
B2_PI = np.float32(3.14159265359)
B2_ANGULAR_SLOP = np.float32(2.0) / np.float32(180.0) * B2_PI          # (2.0f / 180.0f * b2_pi) as a binary32 compiler folds it
EQUAL_T = np.float32(2.0) * B2_ANGULAR_SLOP                            # 2.0f * b2_angularSlop: exact doubling
B2_MAX_TRANSLATION = 2.0
B2_TIME_TO_SLEEP = 0.5
FULL = (180, 60)

Case = collections.namedtuple("Case", "name pop variant schedule kicks")


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


# -------------------------------------------------------------------------------------------------------------- joint variants
EDGE_RUNGS = (np.nextafter(EQUAL_T, np.float32(-1)), EQUAL_T, np.nextafter(EQUAL_T, np.float32(1)))
VARIANTS = ("pi/2", "equal0", "equal_off", "equal_edge", "narrow", "above", "below", "reversed", "wide", "torque0", "torque_big",
            "push")


def edge_rung(ctx):
    """[n_envs, lanes] -> 0 / 1 / 2: which rung of equal_edge a lane's joint takes (spread over joints AND creatures, so that the
    one-joint creatures cover all three as well)."""
    return (np.arange(ctx.K)[None, :] + np.arange(ctx.N)[:, None]) % 3


def apply_variant(morph, variant):
    """-> a copy of `morph` with the variant's joint parameters on every jointed lane."""
    m = morph.take(np.arange(morph.n_envs))
    a = m.arrays
    ctx = Ctx(m)
    j = ctx.jointed.reshape(-1)

    def limits(lo, up):
        a["lower"][j] = _f32(np.broadcast_to(lo, ctx.jointed.shape).reshape(-1)[j])
        a["upper"][j] = _f32(np.broadcast_to(up, ctx.jointed.shape).reshape(-1)[j])

    if variant == "pi/2":
        pass
    elif variant == "equal0":
        limits(0.0, 0.0)
    elif variant == "equal_off":
        limits(0.3, 0.3)
    elif variant == "equal_edge":
        limits(0.0, np.asarray(EDGE_RUNGS, np.float32)[edge_rung(ctx)])
    elif variant == "narrow":
        limits(-0.05, 0.05)
    elif variant == "above":
        limits(0.1, 0.2)
    elif variant == "below":
        limits(-0.2, -0.1)
    elif variant == "reversed":
        limits(0.5, -0.5)
    elif variant == "wide":
        limits(-4.0, 4.0)
    elif variant == "torque0":
        a["torque"][j] = np.float32(0.0)
    elif variant == "torque_big":
        a["torque"][j] = np.float32(1e6)
    elif variant == "push":      # controller value = 0 * sin(..) + offset = +-3 rad: beyond the +-pi/2 limit, the motor pushes into it
        sign = np.where((np.arange(ctx.K)[None, :] + np.arange(ctx.N)[:, None]) % 2 == 0, 3.0, -3.0).reshape(-1)
        a["amp"][j] = 0.0
        a["offset"][j] = sign[j]
    else:
        raise KeyError(variant)
    return m


# ------------------------------------------------------------------------------------------------------------------ schedules
def _dt(x):
    return float(np.float32(x))            # binary64 -> binary32 once; a Python float that ctypes' c_float takes unchanged


def const(fps):
    call = lambda n: (n, _dt(1.0 / fps)) + FULL
    return [call(1)] * 15 + [call(5)] * 4


ALT_FPS = (50, 100, 25, 50, 200, 30, 100, 50, 25, 200)


def alternating():
    return [((1, 2, 3)[i % 3], _dt(1.0 / ALT_FPS[i % len(ALT_FPS)])) + FULL for i in range(18)]


def budget_mix():
    return [(25, _dt(1.0 / 50), 180, 60), (10, _dt(1.0 / 60), 8, 3), (15, _dt(1.0 / 50), 30, 0)]


SCHEDULES = {"const50": const(50), "const60": const(60), "const30": const(30), "const200": const(200), "const10": const(10),
             "alternating": alternating(), "budget_mix": budget_mix()}
KICK_CALLS = (3, 10)


def _cases():
    out = [Case("%s@const50" % v, "lsystem", v, "const50", ()) for v in VARIANTS if v != "pi/2"]
    out += [Case("%s@const50-pairs" % v, "pairs", v, "const50", ()) for v in ("equal_edge", "above")]
    out += [Case("pi/2@%s" % s, "lsystem", "pi/2", s, ()) for s in SCHEDULES if s != "const50"]
    out += [Case("pi/2@const10+kick30", "lsystem", "pi/2", "const10", KICK_CALLS)]
    out += [Case("%s@alternating" % v, "lsystem", v, "alternating", ()) for v in ("equal0", "above", "push")]
    return out


CASES = {c.name: c for c in _cases()}
WIDE_CASES = ("equal0@const50", "push@const50", "pi/2@alternating")


_MORPHS = {}


def case_morphs(case):
    """-> (terrain, [Morphology per lane bucket]) of the case: at most PER_BUCKET creatures per bucket, the variant applied."""
    key = (case.pop, case.variant)
    if key not in _MORPHS:
        terrain, morphs = population(case.pop)
        _MORPHS[key] = (terrain, [apply_variant(m.take(np.arange(min(PER_BUCKET, m.n_envs))), case.variant) for m in morphs])
    return _MORPHS[key]


# ------------------------------------------------------------------------------------------------------------------ the oracle
def new_env(n):
    return dict(reward=np.zeros(n, np.float32), done=np.zeros(n, np.int32), everdone=np.zeros(n, np.int32),
                fitness=np.zeros(n, np.float64), frozen=np.zeros(n, np.int32), steps=np.zeros(n, np.int32))


def env_step(worlds, env, dt, vel_iters, pos_iters):
    """One rem2d_oracle_env_step_ex of every world plus evaluate()'s fitness rule (state_forge.oracle_run's step, with arguments)."""
    for e, w in enumerate(worlds):
        r, d = w.env_step_ex(dt, vel_iters, pos_iters)
        env["reward"][e], env["done"][e] = r, d
        env["everdone"][e] |= d
        if not env["frozen"][e]:
            if r < -10.0:
                env["frozen"][e] = 1
            elif r > 100.0:
                env["fitness"][e], env["frozen"][e] = r + (10000 - env["steps"][e]) / 10000.0, 1
            elif r > 0.0:
                env["fitness"][e] = r
        env["steps"][e] += 1


_RUNS = {}


def oracle_run(O, case, bucket, flags):
    """The oracle's side of a case for one lane bucket -> dict(ctx, reset (snapshot before the first step), every [snapshot after
    every step], ends [index into every of the last step of each call], calls [snapshot after each call], injections {call:
    {field: array}}, speed)."""
    key = (case.name, bucket, flags)
    if key in _RUNS:
        return _RUNS[key]
    terrain, morphs = case_morphs(case)
    morph = morphs[bucket]
    ctx = Ctx(morph, case.pop)
    ot = oracle_terrain(O, terrain)
    md = morph.as_dict()
    worlds = [O.World.from_morph(ot, md, e, flags) for e in range(ctx.N)]
    for e, w in enumerate(worlds):
        assert w.n_bodies == len(ctx.slots[e]) and w.n_joints == len(ctx.slots[e]) - 1
    env = new_env(ctx.N)
    rng = np.random.default_rng([sorted(CASES).index(case.name), ctx.K, flags, 20262])
    run = dict(ctx=ctx, case=case, reset=snapshot(ctx, worlds, env), every=[], ends=[], calls=[], injections={}, speed=0.0)
    snap = run["reset"]
    for c, (n, dt, vi, pi) in enumerate(SCHEDULES[case.schedule]):
        if c in case.kicks:
            inj = F.make_injection("kick30", ctx, snap, rng)
            run["injections"][c] = inj
            assert F.apply_to_oracle(ctx, worlds, snap, inj) > 0
        for _ in range(n):
            env_step(worlds, env, dt, vi, pi)
            snap = snapshot(ctx, worlds, env)
            for f in LANE_FIELDS + SLOT_FIELDS:
                assert np.isfinite(snap[f]).all(), "oracle state not finite: %s %s" % (case.name, f)
            run["every"].append(snap)
            run["speed"] = max(run["speed"], float(np.hypot(snap["vx"], snap["vy"]).max()))
        run["ends"].append(len(run["every"]) - 1)
        run["calls"].append(snap)
    _RUNS[key] = run
    return run


def case_runs(O, case, flags=1):
    return [oracle_run(O, case, b, flags) for b in range(len(case_morphs(case)[1]))]


def left_out(run, pair_slots=24, solver_slots=6):
    """state_forge.left_out over EVERY step of the run (it looks at N_STEPS snapshots at a time) -> (first [n_envs]: index of the
    first CALL in which the oracle shows the creature beyond the build's slots, len(calls) = never; bits [n_envs])."""
    ctx, n = run["ctx"], len(run["every"])
    first, bits = np.full(ctx.N, n, np.int32), np.zeros(ctx.N, np.int32)
    for c0 in range(0, n, F.N_STEPS):
        steps = run["every"][c0:c0 + F.N_STEPS]
        f, b = F.left_out(dict(ctx=ctx, steps=steps), pair_slots, solver_slots)
        new = (f < len(steps)) & (first == n)
        first[new], bits[new] = c0 + f[new], b[new]
    ends = np.asarray(run["ends"])
    return np.searchsorted(ends, first).astype(np.int32), bits     # step s belongs to the first call whose last step is >= s


def n_left_out(runs, pair_slots=24, solver_slots=6):
    return sum(int((left_out(r, pair_slots, solver_slots)[0] < len(r["calls"])).sum()) for r in runs)


# ---------------------------------------------------------------------------------------------------------- what a case reaches
def reach(runs):
    """Counts over all buckets and steps of a case, from the oracle's snapshots alone."""
    out = dict(creatures=0, joint_steps=0, inactive=0, lower=0, upper=0, equal=0, transitions=0, limit_and_motor=0, motor_max=0.0,
               full60=0, asleep=0, toi=0, speed=0.0, pairs=0, steps=0)
    for r in runs:
        ctx = r["ctx"]
        j = ctx.jointed
        out["creatures"] += ctx.N
        out["steps"] = len(r["every"])
        out["speed"] = max(out["speed"], r["speed"])
        out["toi"] += int(r["every"][-1]["toievents"].sum())
        prev = None
        for s in r["every"]:
            lim = s["jlimit"][j]
            out["joint_steps"] += lim.size
            for name, v in (("inactive", 0), ("lower", 1), ("upper", 2), ("equal", 3)):
                out[name] += int((lim == v).sum())
            if prev is not None:
                out["transitions"] += int((lim != prev).sum())
            prev = lim
            at = (lim == LIM_AT_LOWER) | (lim == LIM_AT_UPPER)
            out["limit_and_motor"] += int((at & (s["jmotorimp"][j] != 0)).sum())
            out["motor_max"] = max(out["motor_max"], float(np.abs(s["jmotorimp"][j]).max(initial=0)))
            out["full60"] += int((s["positers"] == 60).sum())
            out["asleep"] += int(((s["awake"] == 0) & ctx.live).sum())
            out["pairs"] = max(out["pairs"], int(s["ccount"].max()))
    out["left_out"] = n_left_out(runs)
    return out


def step_translations(runs):
    """|c(t) - c(t-1)| of every live body over the single-step calls of the runs (binary64 of the binary32 positions)."""
    out = []
    for r in runs:
        sched = SCHEDULES[r["case"].schedule]
        seq = [r["reset"]] + r["calls"]
        for c, (a, b) in enumerate(zip(seq, seq[1:])):
            if sched[c][0] == 1:
                out.append(np.hypot(b["px"].astype(np.float64) - a["px"], b["py"].astype(np.float64) - a["py"])[r["ctx"].live])
    return np.concatenate(out)


# -------------------------------------------------------------------------------------------- binary32 against the binary64 build
def flat_steps(schedule, n_steps=None):
    return [(dt, vi, pi) for n, dt, vi, pi in SCHEDULES[schedule] for _ in range(n)][:n_steps]


def free_flight_chains(variant):
    """tests/test_oracle_f64.py's point-wise population (4 six-module chains spawned 30 m up: joints and motors, no contact) with a
    joint variant -> (flat terrain, [Morphology])."""
    from gym_rem2d_amd import make_terrain, synthetic
    m = synthetic.chain_population(4, 6, "left")
    m.arrays["y"][:] = (m.arrays["y"] + 30.0).astype(np.float32)
    return make_terrain(4, flat=True), [apply_variant(m, variant)]


def truth_trace(O, terrain, morphs, sched, f64):
    """Poses and velocities [steps, bodies of all morphs, 6] of the steps `sched` [(dt, velocity, position iterations)] through the
    binary32 (f64=False) or the binary64 build of the oracle, continuous physics (oracle.World binds the binary32 library only:
    this goes through Terrain.L)."""
    import ctypes as C
    xs, ys, polys = terrain.f32()
    ot = O.Terrain(xs, ys, polys if len(polys) else None, terrain.friction, f64=f64)
    L = ot.L
    rows = []
    for morph in morphs:
        om, keep = O.make_omorph(morph.as_dict())
        per = []
        for e in range(morph.n_envs):
            h = C.c_void_p(L.rem2d_oracle_world_from_morph(ot.h, C.byref(om), e, 1))
            nb = L.rem2d_oracle_num_bodies(h)
            out = np.zeros((nb, 8), np.float32)
            tr = []
            for dt, vi, pi in sched:
                L.rem2d_oracle_env_step_ex(h, dt, vi, pi, None, None)
                L.rem2d_oracle_get_bodies(h, out.ctypes.data_as(C.c_void_p))
                tr.append(out[:, :6].astype(np.float64))
            L.rem2d_oracle_world_destroy(h)
            per.append(np.stack(tr))
        rows.append(np.concatenate(per, axis=1))
    return np.concatenate(rows, axis=1)


if __name__ == "__main__":
    import os
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as O
    O.build()
    print("| case | creatures | steps | joint-steps inactive / lower / upper / equal | transitions | at a limit with motor impulse | "
          "max motor impulse | 60-iteration steps | body-steps asleep | TOI sub-steps | top speed | most pairs | left out |")
    for flags in (1, 0):
        for name, case in CASES.items():
            t0 = time.time()
            st = reach(case_runs(O, case, flags))
            print("| %-22s | %d | %d | %d / %d / %d / %d | %d | %d | %.3g | %d | %d | %d | %.1f | %d | %d |  (flags %d, %.1f s)" % (
                name, st["creatures"], st["steps"], st["inactive"], st["lower"], st["upper"], st["equal"], st["transitions"],
                st["limit_and_motor"], st["motor_max"], st["full60"], st["asleep"], st["toi"], st["speed"], st["pairs"],
                st["left_out"], flags, time.time() - t0))
