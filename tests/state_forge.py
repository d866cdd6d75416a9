"""Injected states: scenarios that put a creature where no trajectory from `reset` takes it, shared by the host half
(tests/test_injected_state_host.py, oracle alone) and the GPU half (tests/test_injected_state_gpu.py).

Protocol (one lane bucket at a time): settle SETTLE steps, inject binary32 values, step N_STEPS more and record the oracle's
whole visible state after every step.  An injection is a dict {arena field name: full [.., n_envs, lanes] array}; only the
entries under the field's mask (live body / jointed body / manifold point that exists) are written -- on the oracle through
set_body_state / set_joint_impulses / set_contact_impulses, on the GPU through ``BatchedWorld.view(name)``.  Both writes
leave fat AABBs, sleep timers, limit states and list order alone.  Everything is drawn from a seeded generator, computed in
binary64 and rounded ONCE to binary32 on the host, so both sides receive the same bits.

What the scenarios reach, oracle alone, L-system population (143 creatures in lane buckets 2/4/8/16, seeds 0..299, rough
terrain seed 4, continuous physics, 15 compared steps = 2 145 creature-steps; `python tests/state_forge.py` prints it):

| scenario   | TOI sub-steps | 60-iteration steps | most pairs on a body | top speed m/s | left out (24 / 6 slots) |
|------------|---------------|--------------------|----------------------|---------------|-------------------------|
| natural    | 185           | 294                | 5                    | 15.2          | 0                       |
| kick3      | 59            | 210                | 5                    | 11.9          | 0                       |
| kick30     | 414           | 630                | 20                   | 84.0          | 0                       |
| kick150    | 888           | 974                | 23                   | 100 (clamp)   | 0 (discrete physics: 1) |
| throw      | 669           | 336                | 7                    | 34.5          | 0                       |
| turns40    | 184           | 279                | 5                    | 15.2          | 0                       |
| turns-1000 | 185           | 387                | 5                    | 15.2          | 0                       |
| spin       | 227           | 326                | 7                    | 33.0          | 0                       |
| impulses   | 188           | 304                | 5                    | 15.2          | 0                       |
| overlap    | 875           | 963                | 7                    | 18.2          | 0                       |
| limit (40 two-body creatures; natural 54 / 21 / 4 / 6.0) | 41 | 22 | 5 | 6.3 | 0                       |

Other populations, continuous physics, natural -> kick150: direct (67 creatures) 79 -> 387 TOI sub-steps, 6 -> 27 pairs, 1
left out; cppn on the hardcore track (117 creatures, top kick 100 m/s) 124 -> 616 TOI sub-steps, 6 -> 25 pairs, 1 left out.
The wide build (32 / 12 slots) leaves nobody out anywhere.  One scenario takes the oracle 0.2 - 0.7 s per population.

On the GPU (MI355X, 150 test ids, about 30 s for the module): 24 525 creature-steps compared per scenario over its 15 ids
(limit: 3 000 over 5), kick150 34 257 over 21 ids (6 of them in the wide build) with 11 creatures left out.

A creature is left out of a comparison only from the step on at which the ORACLE shows one of its bodies with more pairs
than the build's pair slots or more touching contacts than its solver slots (``left_out``); never more than LEFT_OUT_CAP
of a population, and none at all in throw, turns and limit.
"""
import math

import numpy as np

SETTLE = 25
N_STEPS = 15
O_SLOTS = 32                      # O_MAX_BODY_CONTACTS: rows rem2d_oracle_get_contacts can write
LEFT_OUT_CAP = 0.02
NEVER_LEFT_OUT = ("throw", "turns40", "turns-1000", "limit")
ERR_PAIR, ERR_SOLVER, ERR_HANDOVER = 1, 2, 4

BODY_F = ("px", "py", "ang", "vx", "vy", "w")
JOINT_F = ("jimpx", "jimpy", "jimpz", "jmotorimp")
CONTACT_F = ("cn0", "cn1", "ct0", "ct1")
# the oracle's visible state in arena layout: per lane / per pair slot x lane / per creature
LANE_FIELDS = BODY_F + ("sleept", "awake") + JOINT_F + ("jmotorspeed", "jlimit", "ccount")
SLOT_FIELDS = ("cedge", "cnpt", "ctype", "ckey0", "ckey1") + CONTACT_F
ENV_FIELDS = ("positers", "toievents", "reward", "done", "everdone", "fitness", "wod")

# scenario -> steps (0 = right after settling) at which it injects
SCENARIOS = {
    "kick3": (0, 5, 10), "kick30": (0, 5, 10), "kick150": (0, 5, 10), "throw": (0,), "turns40": (0,), "turns-1000": (0,),
    "spin": (0,), "limit": (0,), "impulses": (0, 5, 10), "overlap": (0,),
}
KICK_SIGMA = {"kick3": (3.0, 3.0), "kick30": (30.0, 20.0), "kick150": (150.0, 80.0)}
# on the hardcore track (stairs and stumps: many static boxes under one fat AABB) 150 m/s sends more than LEFT_OUT_CAP of the
# creatures past 24 pairs on a body (4 of 117 on the CPU); the top kick is lowered there until the oracle alone is within it
KICK_SIGMA_TOP = {"cppn": (100.0, 80.0)}
IMPULSE_FACTORS = (0.0, -1.0, 3.0, 50.0)
LIMIT_VARIANTS = ("lower", "lower+ulp", "lower-ulp", "upper", "upper-ulp", "upper+ulp", "lower-0.3", "upper+0.3")


# ---------------------------------------------------------------------------------------------------------------- populations
def _buckets(specs, cap, only=None):
    from gym_rem2d_amd.compiler import Morphology, lanes_for
    groups = {}
    for s in specs:
        k = lanes_for(s.n_bodies)
        if len(groups.setdefault(k, [])) < cap and (only is None or only(s)):
            groups[k].append(s)
    return [Morphology.from_specs(groups[k], k) for k in sorted(groups) if groups[k]]


_POPS = {}


def population(name):
    """name -> (terrain, [Morphology per lane bucket]).  lsystem / direct stand on the rough terrain, cppn is dropped from 0.5 m
    along the hardcore track so that it meets the polygon obstacles; pairs = two-body creatures (lane bucket 2) for `limit`."""
    if name in _POPS:
        return _POPS[name]
    from gym_rem2d_amd import make_terrain, synthetic
    if name == "lsystem":
        pop = (make_terrain(4), _buckets(synthetic.lsystem_specs(range(300)), 40))
    elif name == "pairs":
        pop = (make_terrain(4), _buckets(synthetic.lsystem_specs(range(300)), 40, only=lambda s: s.n_bodies == 2))
    elif name == "direct":
        pop = (make_terrain(4), _buckets(synthetic.direct_specs(range(80)), 30))
    elif name == "cppn":
        terrain = make_terrain(4, hardcore=True)
        morphs = _buckets(synthetic.cppn_specs(range(160)), 40)
        first = float(terrain.polys[:, :, 0].min())
        for m in morphs:
            a, K = m.arrays, m.lanes
            for e in range(m.n_envs):
                sl = slice(e * K, (e + 1) * K)
                live = a["shape"][sl] != 0
                a["x"][sl][live] = (a["x"][sl][live] + np.float32((e % 20) * 1.4 + (first - 7.0))).astype(np.float32)
                a["y"][sl][live] = (a["y"][sl][live] + np.float32(0.5)).astype(np.float32)
        pop = (terrain, morphs)
    else:
        raise KeyError(name)
    _POPS[name] = pop
    return pop


def populations_of(scenario):
    return ("pairs",) if scenario == "limit" else ("lsystem", "direct", "cppn")


def oracle_terrain(O, terrain):
    xs, ys, polys = terrain.f32()
    return O.Terrain(xs, ys, polys if len(polys) else None, terrain.friction)


# ------------------------------------------------------------------------------------------------------------------ the oracle
class Ctx:
    """Layout of one lane bucket: which lanes hold a body, which of those a joint; body / joint index of a lane."""

    def __init__(self, morph, pop=None):
        self.morph, self.pop = morph, pop
        self.N, self.K = morph.n_envs, morph.lanes
        a = morph.arrays
        self.live = (a["shape"] != 0).reshape(self.N, self.K)
        self.parent = a["parent"].reshape(self.N, self.K)
        self.jointed = self.live & (self.parent >= 0)
        self.slots = [np.flatnonzero(self.live[e]) for e in range(self.N)]          # body b of creature e = lane slots[e][b]
        for e in range(self.N):  # joints are created with the bodies: joint q belongs to the q-th jointed lane = body q + 1
            assert self.slots[e][0] == 0 and not self.jointed[e, 0] and self.jointed[e, self.slots[e][1:]].all()

    def field(self, name):
        return self.morph.arrays[name].reshape(self.N, self.K)


def snapshot(ctx, worlds, env):
    """Everything oracle.World exposes, in arena layout.  env: the running per-creature words (reward .. fitness)."""
    N, K = ctx.N, ctx.K
    s = {f: np.zeros((N, K), np.float32) for f in LANE_FIELDS}
    for f in ("awake", "jlimit", "ccount"):
        s[f] = np.zeros((N, K), np.int32)
    for f in SLOT_FIELDS:
        s[f] = np.zeros((O_SLOTS, N, K), np.float32 if f in CONTACT_F else np.int32)
    s["ctouch"] = np.zeros((O_SLOTS, N, K), np.int32)
    s["positers"] = np.array([w.position_iterations for w in worlds], np.int32)
    s["toievents"] = np.array([w.toi_events for w in worlds], np.int32)
    s["wod"] = np.array([w.wod for w in worlds], np.float64)
    for f in ("reward", "done", "everdone", "fitness"):
        s[f] = env[f].copy()
    for e, w in enumerate(worlds):
        sl = ctx.slots[e]
        b = w.bodies()
        for q, f in enumerate(BODY_F + ("sleept",)):
            s[f][e, sl] = b[:, q]
        s["awake"][e, sl] = b[:, 7].astype(np.int32)
        if len(sl) > 1:
            j = w.joints()
            for q, f in enumerate(JOINT_F + ("jmotorspeed",)):
                s[f][e, sl[1:]] = j[:, q]
            s["jlimit"][e, sl[1:]] = j[:, 5].astype(np.int32)
        for bi, lane in enumerate(sl):
            ci, cf = w.contacts(bi)
            n = len(ci)
            s["ccount"][e, lane] = n
            if n:
                s["cedge"][:n, e, lane], s["cnpt"][:n, e, lane], s["ctype"][:n, e, lane] = ci[:, 0], ci[:, 1], ci[:, 2]
                s["ctouch"][:n, e, lane], s["ckey0"][:n, e, lane], s["ckey1"][:n, e, lane] = ci[:, 3], ci[:, 4], ci[:, 5]
                for q, f in enumerate(CONTACT_F):
                    s[f][:n, e, lane] = cf[:, q]
    return s


def masks(ctx, snap):
    """Which entries of a field mean something: field name -> bool array of the field's shape."""
    k = np.arange(O_SLOTS)[:, None, None]
    pair = ctx.live[None] & (k < snap["ccount"][None])
    m = {f: ctx.live for f in BODY_F + ("sleept", "awake", "ccount")}
    m.update({f: ctx.jointed for f in JOINT_F + ("jmotorspeed", "jlimit")})
    m.update(cedge=pair, cnpt=pair, ctype=pair & (snap["cnpt"] > 0))
    for j in (0, 1):
        for f in ("ckey%d", "cn%d", "ct%d"):
            m[f % j] = pair & (snap["cnpt"] > j)
    return m


def apply_to_oracle(ctx, worlds, snap, inj):
    """Write the injection into the oracle worlds; returns how many written values differ from the state they replace."""
    new = dict(snap)
    msk = masks(ctx, snap)
    changed = 0
    for f, v in inj.items():
        assert v.dtype == snap[f].dtype and v.shape == snap[f].shape and np.isfinite(v[msk[f]]).all(), f
        new[f] = np.where(msk[f], v, snap[f])
        changed += int((new[f] != snap[f]).sum())
    body = any(f in inj for f in BODY_F + ("awake",))
    joint = any(f in inj for f in JOINT_F)
    contact = any(f in inj for f in CONTACT_F)
    for e, w in enumerate(worlds):
        sl = ctx.slots[e]
        for bi, lane in enumerate(sl):
            if body:
                w.set_body_state(bi, *[float(new[f][e, lane]) for f in BODY_F], awake=int(new["awake"][e, lane]))
            if joint and bi > 0:
                w.set_joint_impulses(bi - 1, *[float(new[f][e, lane]) for f in JOINT_F])
            if contact:
                for k in range(int(snap["ccount"][e, lane])):
                    w.set_contact_impulses(bi, k, *[float(new[f][k, e, lane]) for f in CONTACT_F])
    return changed


# ------------------------------------------------------------------------------------------------------------------- scenarios
def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def make_injection(scenario, ctx, snap, rng):
    """The values a scenario writes, from the state it finds: {field: full array}.  Entries outside the field's mask are
    ignored.  Every scenario that writes a body also writes awake = 1 (b2Body::SetTransform / SetLinearVelocity wake)."""
    N, K = ctx.N, ctx.K
    awake = np.ones((N, K), np.int32)
    if scenario in KICK_SIGMA:       # 1. pose kept, (vx, vy, w) ~ N(0, sigma)
        sv, sw = KICK_SIGMA_TOP.get(ctx.pop, KICK_SIGMA[scenario]) if scenario == "kick150" else KICK_SIGMA[scenario]
        return dict(vx=_f32(rng.normal(0, sv, (N, K))), vy=_f32(rng.normal(0, sv, (N, K))), w=_f32(rng.normal(0, sw, (N, K))),
                    awake=awake)
    if scenario == "throw":          # 2. rotated about the root, lifted 6 m, thrown down at 25 m/s
        th = rng.uniform(-math.pi, math.pi, (N, 1))
        c, s = np.cos(th), np.sin(th)
        dx = snap["px"].astype(np.float64) - snap["px"][:, :1]
        dy = snap["py"].astype(np.float64) - snap["py"][:, :1]
        return dict(px=_f32(snap["px"][:, :1] + c * dx - s * dy), py=_f32(snap["py"][:, :1] + s * dx + c * dy + 6.0),
                    ang=_f32(snap["ang"] + th), vx=np.zeros((N, K), np.float32), vy=np.full((N, K), -25.0, np.float32),
                    w=np.zeros((N, K), np.float32), awake=awake)
    if scenario in ("turns40", "turns-1000"):   # 3. whole turns: the kernels' own sine / cosine range reduction
        turns = 40.0 if scenario == "turns40" else -1000.0
        return dict(ang=_f32(snap["ang"].astype(np.float64) + 2.0 * math.pi * turns), awake=awake)
    if scenario == "spin":           # 4. b2_maxRotation clamp, circle-on-ground friction at speed
        sign = np.where(rng.random((N, K)) < 0.5, -1.0, 1.0)
        return dict(w=_f32(200.0 * sign), awake=awake)
    if scenario == "limit":          # 5. two bodies: root set upright (angle 0), child turned about the joint anchor
        assert K == 2
        lower, upper = ctx.field("lower")[:, 1], ctx.field("upper")[:, 1]
        inf = np.float32(np.inf)
        target = np.zeros(N, np.float32)
        for e in range(N):
            lo, up = lower[e], upper[e]
            target[e] = {"lower": lo, "lower+ulp": np.nextafter(lo, inf), "lower-ulp": np.nextafter(lo, -inf), "upper": up,
                         "upper-ulp": np.nextafter(up, -inf), "upper+ulp": np.nextafter(up, inf),
                         "lower-0.3": np.float32(lo - np.float32(0.3)), "upper+0.3": np.float32(up + np.float32(0.3))
                         }[LIMIT_VARIANTS[e % len(LIMIT_VARIANTS)]]
        ang = np.zeros((N, 2), np.float32)
        ang[:, 1] = target                       # joint angle = aB - aA - 0 = target - 0: exact
        t = target.astype(np.float64)
        ax, ay, bx, by = (ctx.field(f)[:, 1].astype(np.float64) for f in ("ax", "ay", "bx", "by"))
        px, py = snap["px"].astype(np.float64), snap["py"].astype(np.float64)
        px[:, 1] = px[:, 0] + ax - (np.cos(t) * bx - np.sin(t) * by)
        py[:, 1] = py[:, 0] + ay - (np.sin(t) * bx + np.cos(t) * by)
        return dict(px=_f32(px), py=_f32(py), ang=ang, awake=awake)
    if scenario == "impulses":       # 6. warm-start state scaled, one factor per creature
        fac = np.float32(IMPULSE_FACTORS)[rng.integers(0, len(IMPULSE_FACTORS), N)]
        out = {f: (snap[f] * fac[:, None]).astype(np.float32) for f in JOINT_F}
        out.update({f: (snap[f] * fac[None, :, None]).astype(np.float32) for f in CONTACT_F})
        return out
    if scenario == "overlap":        # 7. half a root-module height into the ground, pose only
        shape, hx, hy = ctx.field("shape")[:, 0], ctx.field("hx")[:, 0], ctx.field("hy")[:, 0]
        height = 2.0 * np.where(shape == 2, hx, hy).astype(np.float64)
        return dict(py=_f32(snap["py"] - 0.5 * height[:, None]), awake=awake)
    raise KeyError(scenario)


def negative_normal_injection(scenario, ctx, snap, rng):
    """The reduced case of what `impulses` found: every normal impulse negated, nothing else.  friction * normalImpulse is then
    a NEGATIVE friction bound in the first velocity iteration, where b2Clamp(a, -m, m) = b2Max(-m, b2Min(a, m)) = -m."""
    return {f: (-snap[f]).astype(np.float32) for f in ("cn0", "cn1")}


def noop_injection(scenario, ctx, snap, rng):
    """What a scenario turns into if its injection is lost: the self-check of the host half uses it to show that its own
    assertions then fail."""
    return {}


# ---------------------------------------------------------------------------------------------------------------- the protocol
def _seed(scenario, pop, K, flags):
    return [sorted(SCENARIOS).index(scenario), ("lsystem", "pairs", "direct", "cppn").index(pop), K, flags, 20261]


_RUNS = {}


def oracle_run(O, pop, bucket, scenario, flags, make=make_injection):
    """The oracle's side of the protocol for lane bucket `bucket` of population `pop`; scenario None = the un-injected run.
    -> dict(ctx, settled, injections {step: {field: array}}, steps [snapshot after step 1..N_STEPS], changed, speed)."""
    key = (pop, bucket, scenario, flags, make.__name__)
    if key in _RUNS:
        return _RUNS[key]
    terrain, morphs = population(pop)
    morph = morphs[bucket]
    ctx = Ctx(morph, pop)
    ot = oracle_terrain(O, terrain)
    md = morph.as_dict()
    worlds = [O.World.from_morph(ot, md, e, flags) for e in range(ctx.N)]
    for e, w in enumerate(worlds):  # oracle body b is lane slots[e][b]: the creation pose says so
        b, sl = w.bodies(), ctx.slots[e]
        assert w.n_bodies == len(sl) and w.n_joints == len(sl) - 1
        assert all(np.array_equal(b[:, q], ctx.field(f)[e, sl]) for q, f in enumerate(("x", "y", "angle")))
    env = dict(reward=np.zeros(ctx.N, np.float32), done=np.zeros(ctx.N, np.int32), everdone=np.zeros(ctx.N, np.int32),
               fitness=np.zeros(ctx.N, np.float64), frozen=np.zeros(ctx.N, np.int32), steps=np.zeros(ctx.N, np.int32))

    def step():
        for e, w in enumerate(worlds):
            r, d = w.env_step()
            env["reward"][e], env["done"][e] = r, d
            env["everdone"][e] |= d
            if not env["frozen"][e]:    # evaluate()'s fitness rule, as in rem2d_oracle_batch_run
                if r < -10.0:
                    env["frozen"][e] = 1
                elif r > 100.0:
                    env["fitness"][e], env["frozen"][e] = r + (10000 - env["steps"][e]) / 10000.0, 1
                elif r > 0.0:
                    env["fitness"][e] = r
            env["steps"][e] += 1

    for _ in range(SETTLE):
        step()
    rng = np.random.default_rng(_seed(scenario or "kick3", pop, ctx.K, flags))
    run = dict(ctx=ctx, settled=snapshot(ctx, worlds, env), injections={}, steps=[], changed=0, speed=0.0)
    snap = run["settled"]
    for t in range(N_STEPS):
        if scenario is not None and t in SCENARIOS[scenario]:
            inj = make(scenario, ctx, snap, rng)
            run["injections"][t] = inj
            run["changed"] += apply_to_oracle(ctx, worlds, snap, inj)
        step()
        snap = snapshot(ctx, worlds, env)
        for f in LANE_FIELDS + SLOT_FIELDS:
            assert np.isfinite(snap[f]).all(), "oracle state not finite: %s %s step %d" % (scenario, f, t + 1)
        run["steps"].append(snap)
        run["speed"] = max(run["speed"], float(np.hypot(snap["vx"], snap["vy"]).max()))
    _RUNS[key] = run
    return run


def left_out(run, pair_slots=24, solver_slots=6):
    """-> (first [n_envs]: index into run["steps"] from which the creature is left out, N_STEPS = never; bits [n_envs]: the
    capacity bit(s) the oracle's own state justifies at that step)."""
    ctx = run["ctx"]
    first, bits = np.full(ctx.N, N_STEPS, np.int32), np.zeros(ctx.N, np.int32)
    for t, s in enumerate(run["steps"]):
        pairs = s["ccount"].max(axis=1)
        touch = ((s["ctouch"] != 0) & masks(ctx, s)["cedge"]).sum(axis=0).max(axis=1)
        b = np.where(pairs > pair_slots, ERR_PAIR, 0) | np.where(touch > solver_slots, ERR_SOLVER, 0)
        new = (b != 0) & (first == N_STEPS)
        first[new], bits[new] = t, b[new]
    return first, bits


def stats(run):
    """(TOI sub-steps, creature-steps that used all 60 position iterations, most pairs on a body, top speed) of the compared
    steps."""
    toi = int((run["steps"][-1]["toievents"] - run["settled"]["toievents"]).sum())
    full = int(sum((s["positers"] == 60).sum() for s in run["steps"]))
    pairs = int(max(s["ccount"].max() for s in run["steps"]))
    return toi, full, pairs, run["speed"]


def population_runs(O, pop, scenario, flags, make=make_injection):
    return [oracle_run(O, pop, b, scenario, flags, make) for b in range(len(population(pop)[1]))]


def population_stats(runs, pair_slots=24, solver_slots=6):
    toi = full = pairs = out = n = 0
    speed = 0.0
    for r in runs:
        a, b, c, d = stats(r)
        toi, full, pairs, speed = toi + a, full + b, max(pairs, c), max(speed, d)
        out += int((left_out(r, pair_slots, solver_slots)[0] < N_STEPS).sum())
        n += r["ctx"].N
    return dict(creatures=n, toi=toi, full60=full, pairs=pairs, speed=speed, left_out=out)


def check_left_out_cap(scenario, runs, pair_slots=24, solver_slots=6):
    st = population_stats(runs, pair_slots, solver_slots)
    cap = 0 if scenario in NEVER_LEFT_OUT else int(LEFT_OUT_CAP * st["creatures"])
    assert st["left_out"] <= cap, "%s leaves out %d of %d creatures (cap %d)" % (scenario, st["left_out"], st["creatures"], cap)
    return st


if __name__ == "__main__":
    import os
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as O
    O.build()
    for pop in ("lsystem", "direct", "cppn", "pairs"):
        for flags in (1, 0):
            print("| %s flags %d | creatures | TOI sub-steps | 60-iteration steps | most pairs | top speed | left out |" % (pop, flags))
            for sc in [None] + list(SCENARIOS):
                if (sc == "limit") != (pop == "pairs") and sc is not None:
                    continue
                t0 = time.time()
                st = population_stats(population_runs(O, pop, sc, flags))
                print("| %-10s | %d | %d | %d | %d | %.1f | %d |  (%.1f s)" % (sc or "natural", st["creatures"], st["toi"], st["full60"],
                                                                       st["pairs"], st["speed"], st["left_out"], time.time() - t0))
