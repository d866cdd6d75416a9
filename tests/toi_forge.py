"""Forged scenes for the TOI event loop (csrc/rem2d_toi.h solve_toi_lane) at every lanes-per-body form, shared by the host half
(tests/test_toi_forms_host.py, oracle alone) and the GPU half (tests/test_toi_forms_gpu.py).

rem2d_toi_heavy_multi_kernel deals the TOI work list out `per = max(heavy_per_wave, ceil(queued / blocks))` bodies to a wavefront and
gives each body G lanes, G the largest power of two with G * per <= 64 (csrc/rem2d_kernels.h toi_heavy_body; `lanes_per_body` below
restates it).  G decides the shape of the loop: the alpha pass deals the pair slots sub, sub + G, ... to the body's lanes and
reduces (smallest alpha, first slot among equals) across them; the velocity sweeps of a sub-step take the quad form for G >= 4 and
the serial form below; either sends constraints beyond the third through scratch.  A scene is a few small creatures PLACED over a
forged polyline (terrain_forge.place), given a velocity before the first step (an injection of state_forge's kind: vx, vy, w, awake,
written on the oracle through set_body_state and on the GPU through the arena views) and stepped for a few steps.  Each scene
states the branch it is for, and the host half proves on the ORACLE that the branch is met (`reach`):

  ladder      one- and two-body creatures (boxes, circles, a box with a circle) thrown down on flat and on sawtooth ground.  Built at
              every lane count K, so that heavy_per_wave = h with a body density of at most h / 64 pins G = 64 / h.
  crowd       replicas at one height: every body queues in the landing step, and the QUEUE LENGTH alone forces G = 4 (one body in
              4 lanes), 2 (one body in 2 lanes), 1 (a flat two-chain in 2 lanes) under the default heavy_per_wave = 1.  crowd-odd: 131 of
              256 four-lane creatures land, the others hang 6 m up without a pair: per = 9 over 16 blocks, so slots 9 .. 15 of a
              wavefront, the tail of block 14 and all of block 15 take the kernel's three early exits.
  many pairs  a 1 x 1 box and an r = 0.5 circle arriving fast and slanted on polylines of pitch 0.1: more pairs on a body than
              lanes at G <= 8 (a lane takes several slots), resting across four to six short edges (a sub-step island beyond the three
              constraints kept in registers).  `manypairs-wide`: more than six manifolds, compared in the wide build only.
  tie         a box arriving flat across the joint of two collinear edges, and across the top corner of a static box level with the
              edge beside it: pairs of one body with the SAME minimal alpha in one alpha pass; the first in list order wins.
  repeat      bodies driven into V notches and a stair corner: several TOI events of one body within one step.
  flags       a ladder and a crowd scene under CONTINUOUS | SLEEP_RESET_ALWAYS with every second creature asleep at injection.

`python tests/toi_forge.py` prints the table of DESIGN.md section 9 (TOI forms) from the oracle.
"""
import collections

import numpy as np

import state_forge as F
import terrain_forge as G

CONT, SLEEP_RESET_ALWAYS = 1, 2
WAVE = 64
KR = 3                                  # constraints of a sub-step island kept in registers (csrc: KR); further ones go through scratch
CAPACITY = {False: (24, 6), True: (32, 12)}     # (pair slots, solver slots) of the default / the wide build

Scene = collections.namedtuple("Scene", "name branch terrain morph inj flags steps low wide_only")


# ------------------------------------------------------------------------------------------------- the kernel's dealing, restated
def lanes_per_body(heavy_per_wave, Lp, queued):
    """(per, G) of toi_heavy_body for a world of Lp lanes with `queued` bodies on the work list (queued > 0)."""
    blocks = Lp // WAVE
    per = max(int(heavy_per_wave), (queued + blocks - 1) // blocks)
    g = 1
    while g * 2 * per <= WAVE:
        g *= 2
    return per, g


def guaranteed_G(heavy_per_wave, Lp, lower, upper):
    """The G every launch with lower <= queued <= upper takes, or None where the bounds allow more than one (G falls as the
    queue grows, so the two ends decide)."""
    if lower <= 0:
        return None
    a, b = lanes_per_body(heavy_per_wave, Lp, lower)[1], lanes_per_body(heavy_per_wave, Lp, upper)[1]
    return a if a == b else None


# -------------------------------------------------------------------------------------------------------------------- creatures
def _spec(kind):
    """One creature at the origin.  box / flatbox / tallbox / bigbox / circle / bigcircle: one body; chain: two boxes side by side on a
    revolute joint (lying flat: both land in the same step); cart: a box with a circle hung on its right."""
    from gym_rem2d_amd.compiler import CreatureBuilder, CreatureSpec
    b = CreatureBuilder()
    if kind == "box":
        b.add_box(0.3, 0.2, 0.0, 0.0, 0.0)
    elif kind == "flatbox":
        b.add_box(0.5, 0.15, 0.0, 0.0, 0.0)
    elif kind == "tallbox":
        b.add_box(0.12, 0.4, 0.0, 0.0, 0.0)
    elif kind == "bigbox":
        b.add_box(0.5, 0.5, 0.0, 0.0, 0.0)
    elif kind == "circle":
        b.add_circle(0.25, 0.0, 0.0, 0.0)
    elif kind == "bigcircle":
        b.add_circle(0.5, 0.0, 0.0, 0.0)
    elif kind == "chain":
        p, c = b.add_box(0.3, 0.15, 0.0, 0.0, 0.0), b.add_box(0.3, 0.15, 0.6, 0.0, 0.0)
        b.add_revolute(p, c, (0.3, 0.0), (-0.3, 0.0), 50.0)
    elif kind == "cart":
        p, c = b.add_box(0.3, 0.2, 0.0, 0.0, 0.0), b.add_circle(0.2, 0.5, 0.0, 0.0)
        b.add_revolute(p, c, (0.5, 0.0), (0.0, 0.0), 50.0)
    else:
        raise KeyError(kind)
    return CreatureSpec(b, [])


def _morph(kinds, lanes):
    from gym_rem2d_amd.compiler import Morphology
    specs = {k: _spec(k) for k in set(kinds)}
    return Morphology.from_specs([specs[k] for k in kinds], lanes)


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _injection(morph, vx, vy, w, asleep=None):
    """The call-0 injection: every live body of creature e gets (vx[e], vy[e], w[e]); awake = 1, or 0 for the creatures in `asleep`."""
    N, K = morph.n_envs, morph.lanes
    full = lambda v: np.repeat(_f32(np.broadcast_to(v, (N,)))[:, None], K, axis=1)      # noqa: E731
    awake = np.ones((N, K), np.int32)
    if asleep is not None:
        awake[np.asarray(asleep, bool)] = 0
    return dict(vx=full(vx), vy=full(vy), w=full(w), awake=awake)


# --------------------------------------------------------------------------------------------------------------------- terrains
def _T():
    from gym_rem2d_amd import terrain
    return terrain


def flat(n=200, y=5.0):
    T = _T()
    return T.TerrainProfile(T.TERRAIN_STEP * np.arange(n), np.full(n, y), [])


def arcs(curv_hump, curv_bowl=1.0 / 0.53, pitch=0.1, n=200, y=5.0, period=4.0):
    """Pitch-0.1 polyline of parabolic arcs about the centres period * (k + 1/2): humps y + curv_hump * d^2 / 2 in the even
    periods (a flat box touches only the edges at the top), bowls y + min(curv_bowl * d^2 / 2, 0.5) in the odd ones (a circle of
    radius near 1 / curv_bowl touches many edges at the bottom)."""
    xs = pitch * np.arange(n)
    d = (xs % period) - period / 2.0
    even = (xs // period).astype(int) % 2 == 0
    return _T().TerrainProfile(xs, y + np.where(even, 0.5 * curv_hump * d * d, np.minimum(0.5 * curv_bowl * d * d, 0.5)), [])


def notches(n=400, pitch=0.25):
    """Flat ground of pitch 0.25 with V notches two edges wide, 0.7 .. 2 m deep (walls of slope 2.8 .. 8), every second one
    followed by a stair corner: a riser of one edge, a tread of four."""
    ys = np.full(n, 6.0)
    for k, i in enumerate(range(10, n - 10, 10)):
        ys[i] -= (0.7, 2.0, 1.0, 1.4)[k % 4]      # the tip of the V is point i
        if k % 2:
            ys[i + 4:i + 9] += 0.5
    return _T().TerrainProfile(pitch * np.arange(n), ys, [])


def ledge():
    """Flat ground at y = 5 with static boxes standing on it whose tops (y = 5.5) are level with a raised stretch of the polyline
    that begins at their right side: a body across that corner rests on a static box and on an edge of one height."""
    T = _T()
    p = T.TERRAIN_STEP
    n = 200
    ys = np.full(n, 5.0)
    polys = []
    for i in range(10, n - 10, 10):
        ys[i:i + 5] = 5.5                        # raised from point i (the riser is edge i - 1) to point i + 4
        x = i * p
        polys.append([(x - 2 * p, 5.0), (x, 5.0), (x, 5.5), (x - 2 * p, 5.5)])
    return T.TerrainProfile(p * np.arange(n), ys, polys)


_TERRAINS = {"flat": flat, "saw": lambda: G.sawtooth(200, _T().TERRAIN_STEP, 0.0, deltas=(0.03, 0.1, 0.2, 0.4)),
             "arcs": lambda: arcs(-0.45), "arcs_wide": lambda: arcs(-0.12, 1.0 / 0.51),
             "notches": notches, "ledge": ledge}
_PROFILES = {}


def profile(name):
    if name not in _PROFILES:
        _PROFILES[name] = _TERRAINS[name]()
    return _PROFILES[name]


# ----------------------------------------------------------------------------------------------------------------------- scenes
LADDER = {1: 64, 2: 64, 4: 32, 8: 16, 16: 8, 32: 4, 64: 2}         # heavy_per_wave -> K: a body density of at most h / 64
N_LADDER = 64


def _ladder(h, ground, flags=CONT, asleep=False):
    """64 creatures in K = LADDER[h] lanes: one body each for h = 1 (density 1 / 64), else one- and two-body creatures in turn
    (density at most 2 / K = h / 64).  Thrown down at 6 .. 12 m/s, some slanted and spinning, from 0.25 m: they land in steps 1 .. 4."""
    K = LADDER[h]
    kinds = [("box", "circle", "flatbox")[e % 3] if h == 1 else ("box", "chain", "circle", "cart")[e % 4] for e in range(N_LADDER)]
    m = _morph(kinds, K)
    prof = profile(ground)
    e = np.arange(N_LADDER)
    m = G.place(m, prof, 4.0 + (prof.xs[-1] - 10.0) * (e + 0.31) / N_LADDER, clearance=0.25)
    inj = _injection(m, vx=(e % 5 - 2) * 1.5, vy=-6.0 - (e % 7), w=(e % 3 - 1) * 2.0, asleep=((e % 4 == 1) | (e % 4 == 2)) if asleep else None)
    name = "ladder-h%d-K%d-%s%s" % (h, K, ground, "-sleep" if asleep else "")
    return Scene(name, "flags" if asleep else "ladder", ground, m, inj, flags, 12, np.ones(N_LADDER, bool), False)


CROWDS = {"crowd-G4": ("box", 4, 64, 64), "crowd-G2": ("circle", 2, 64, 64), "crowd-G1": ("chain", 2, 64, 64),
          "crowd-odd": ("box", 4, 256, 131)}


def _crowd(name):
    """Replicas over flat ground at one height with one velocity: every body of the first `low` creatures lands in the same step
    (x differs, so the pairs do); the other creatures are lifted 6 m and meet nothing within the run."""
    kind, K, n, low = CROWDS[name]
    m = _morph([kind] * n, K)
    e = np.arange(n)
    m = G.place(m, profile("flat"), 5.0 + 70.0 * (e + 0.17) / n, clearance=0.3)
    lowm = e < low
    live = m.arrays["shape"] != 0
    m.arrays["y"][live] = (m.arrays["y"] + np.repeat(np.where(lowm, 0.0, 6.0), K).astype(np.float32))[live]
    inj = _injection(m, vx=0.0, vy=-8.0, w=0.0)
    return Scene(name, "crowd", "flat", m, inj, CONT, 10, lowm, False)


N_SMALL = 64
SMALL_K = {64: (1, 64), 8: (8, 8), 4: (16, 4), 2: (32, 2), 1: (64, 2)}     # G -> (heavy_per_wave, K): 64 one-body creatures, density 1 / K


def _shifted_back(m, inj, t=0.02):
    """Move every creature back along its injected velocity by t seconds, so that a slanted throw arrives where it was placed."""
    a = m.arrays
    live = a["shape"] != 0
    a["x"][live] = (a["x"][live].astype(np.float64) - t * inj["vx"].reshape(-1)[live]).astype(np.float32)
    return m


def _manypairs(K, wide):
    """1 x 1 boxes over humps and r = 0.5 circles over bowls of pitch 0.1, arriving at 14 m/s slanted: the swept fat AABB spans
    a dozen and more edges; they come to rest across the few edges at the top of a hump / the bottom of a bowl."""
    m = _morph(["bigbox", "bigcircle"] * (N_SMALL // 2), K)
    ground = "arcs_wide" if wide else "arcs"
    e = np.arange(N_SMALL)
    centre = 2.0 + 4.0 * (2 * ((e // 2) % 2) + (e % 2))            # periods 0 / 2: humps (boxes), 1 / 3: bowls (circles)
    m = G.place(m, profile(ground), centre + ((e // 4) % 4 - 1.5) * 0.02, clearance=0.2)
    inj = _injection(m, vx=np.where(e % 4 < 2, 7.0, -7.0), vy=-12.0, w=0.0)
    m = _shifted_back(m, inj)
    return Scene("manypairs-%sK%d" % ("wide-" if wide else "", K), "many pairs", ground, m, inj, CONT, 25, np.ones(N_SMALL, bool), wide)


def _tie(K):
    """Flat boxes falling straight across a polyline point of flat ground (even creatures), and across the corner where a static
    box's top meets a raised edge of the same height (odd creatures)."""
    p = _T().TERRAIN_STEP
    m = _morph(["flatbox"] * N_SMALL, K)
    e = np.arange(N_SMALL)
    x = np.where(e % 2 == 1, 10, 16) * p + 10 * (e // 2 % 18) * p + ((e // 2) % 3 - 1) * 0.05
    m = G.place(m, profile("ledge"), x, clearance=0.2)
    inj = _injection(m, vx=0.0, vy=-5.0 - (e % 4), w=0.0)
    return Scene("tie-K%d" % K, "tie", "ledge", m, inj, CONT, 10, np.ones(N_SMALL, bool), False)


def _repeat(K):
    """Boxes (turned a little), circles and tall boxes thrown at 20 .. 40 m/s into V notches and stair corners: wall after wall within
    one step.  Every second tall box plunges upright into one of the 2 m deep notches (one PAIR takes several events in a step), the
    others arrive turned and spinning at 80 rad/s."""
    m = _morph(["box", "circle", "tallbox"] * (N_SMALL // 3) + ["tallbox"], K)
    prof = profile("notches")
    e = np.arange(N_SMALL)
    tall, plunge = e % 3 == 2, (e % 3 == 2) & ((e // 3) % 2 == 0)
    m.arrays["angle"][::K] = _f32(np.where(e % 3 == 0, 0.2 + 0.1 * (e % 7), np.where(tall & ~plunge, 0.4, 0.0)))
    notch = np.where(plunge, 20 + 40 * ((e // 6) % 9), 10 * (1 + e % 38))
    m = G.place(m, prof, prof.xs[notch] + np.where(plunge, ((e // 6) % 3) * 0.06, (e % 3 - 1) * 0.02), clearance=0.1)
    inj = _injection(m, vx=np.where(tall, 0.0, np.where(e % 4 < 2, 12.0, -12.0)),
                     vy=np.where(plunge, -20.0 - 10.0 * ((e // 6) % 4), -25.0 - 5.0 * (e % 4)),
                     w=np.where(plunge, 40.0 * ((e // 6) % 2), np.where(tall, 80.0, (e % 5 - 2) * 3.0)))
    m = _shifted_back(m, inj, t=0.01)
    return Scene("repeat-K%d" % K, "repeat", "notches", m, inj, CONT, 30, np.ones(N_SMALL, bool), False)


def _sleepers(K):
    """The flags crowd: 64 one-body creatures (boxes and circles) at one height over flat ground, every second one asleep at
    injection, under CONTINUOUS | SLEEP_RESET_ALWAYS."""
    m = _morph(["box", "box", "circle", "circle"] * (N_SMALL // 4), K)
    e = np.arange(N_SMALL)
    m = G.place(m, profile("flat"), 5.0 + 70.0 * (e + 0.17) / N_SMALL, clearance=0.3)
    inj = _injection(m, vx=0.0, vy=-8.0, w=0.0, asleep=e % 2 == 1)
    return Scene("sleepers-K%d" % K, "flags", "flat", m, inj, CONT | SLEEP_RESET_ALWAYS, 12, np.ones(N_SMALL, bool), False)


_SCENES = {}


def scene(name):
    if name in _SCENES:
        return _SCENES[name]
    part = name.split("-")
    K = int(part[-1][1:]) if part[-1][0] == "K" else None
    if part[0] == "ladder":
        sleep = part[-1] == "sleep"
        s = _ladder(int(part[1][1:]), part[3], CONT | SLEEP_RESET_ALWAYS if sleep else CONT, sleep)
    elif part[0] == "crowd":
        s = _crowd(name)
    elif part[0] == "manypairs":
        s = _manypairs(K, part[1] == "wide")
    else:
        s = {"tie": _tie, "repeat": _repeat, "sleepers": _sleepers}[part[0]](K)
    assert s.name == name, (s.name, name)
    _SCENES[name] = s
    return s


def ladder_name(h, sleep=False):
    return "ladder-h%d-K%d-%s%s" % (h, LADDER[h], "saw" if sleep or h in (1, 4, 16, 64) else "flat", "-sleep" if sleep else "")


LADDER_SCENES = [ladder_name(h) for h in LADDER]
SMALL = ("manypairs", "tie", "repeat", "sleepers")                       # + the flags ladder: run at G in {64, 8, 4, 2, 1} by option


def small_scenes(G_):
    """The many pairs, tie, repeat and flags scenes built for lanes-per-body G_ by option -> (heavy_per_wave, [scene names])."""
    h, K = SMALL_K[G_]
    return h, ["%s-K%d" % (n, K) for n in SMALL] + [ladder_name(h, sleep=True)]


ALL_SCENES = (LADDER_SCENES + list(CROWDS) + sorted({n for g in SMALL_K for n in small_scenes(g)[1]})
              + ["manypairs-wide-K%d" % K for K in sorted({k for _, k in SMALL_K.values()})])


Case = collections.namedtuple("Case", "scene form heavy wide G")     # heavy None: default options; G None: a step train (COLS = 1)
PER_STEP_FORMS = ("velpost", "two_launches", "fused_step_kernel")     # the launch forms that run rem2d_toi_heavy_multi_kernel
TRAINS = ("step_train", "train_128_lanes")
CROWD_G = {"crowd-G4": 4, "crowd-G2": 2, "crowd-G1": 1, "crowd-odd": 4}
WIDE_LADDER = (64, 32, 4)                                             # heavy_per_wave of G = 1, 2, 16


def gpu_cases():
    out = [Case(ladder_name(h), f, h, False, WAVE // h) for h in LADDER for f in PER_STEP_FORMS]
    out += [Case(ladder_name(h), f, h, True, WAVE // h) for h in WIDE_LADDER for f in PER_STEP_FORMS]
    out += [Case(n, f, None, False, g) for n, g in CROWD_G.items() for f in PER_STEP_FORMS]
    out += [Case(n, f, None, False, None) for n in CROWD_G for f in TRAINS]
    for g in SMALL_K:
        h, names = small_scenes(g)
        out += [Case(n, "velpost", h, False, g) for n in names]
        out.append(Case("manypairs-wide-K%d" % SMALL_K[g][1], "velpost", h, True, g))
    out += [Case(n, f, None, False, None) for n in small_scenes(1)[1] for f in TRAINS]
    out.append(Case("manypairs-wide-K2", "step_train", None, True, None))
    return out


def case_id(c):
    return "%s-%s-%s%s" % (c.scene, c.form, "train" if c.G is None else "G%d" % c.G, "-wide" if c.wide else "")


# ------------------------------------------------------------------------------------------------------------------- the oracle
_RUNS = {}


def oracle_run(O, name, inject=True):
    """The oracle's side of a scene: reset, the injection, `steps` single steps.  -> dict(scene, ctx, profile, reset, injections,
    steps [snapshot after every step], events [steps, n_envs] TOI events per creature and step, bodies [steps]: bodies with an event
    in that step, ties [steps, n_envs], count_max / count_skips / island_max [steps]: rem2d_oracle_toi_counters, summed / maximised over the worlds).
    inject=False: the un-injected run from the same reset (what the oracle-backed twin of the ABI can replay)."""
    key = (name, inject)
    if key in _RUNS:
        return _RUNS[key]
    s = scene(name)
    prof, ctx = profile(s.terrain), F.Ctx(s.morph, name)
    ot = F.oracle_terrain(O, prof)
    md = s.morph.as_dict()
    worlds = [O.World.from_morph(ot, md, e, s.flags) for e in range(ctx.N)]
    for e, w in enumerate(worlds):
        assert w.n_bodies == len(ctx.slots[e]) and w.n_joints == len(ctx.slots[e]) - 1
    env = dict(reward=np.zeros(ctx.N, np.float32), done=np.zeros(ctx.N, np.int32), everdone=np.zeros(ctx.N, np.int32),
               fitness=np.zeros(ctx.N, np.float64), frozen=np.zeros(ctx.N, np.int32), steps=np.zeros(ctx.N, np.int32))
    run = dict(scene=s, ctx=ctx, profile=prof, reset=F.snapshot(ctx, worlds, env), injections={}, steps=[],
               events=np.zeros((s.steps, ctx.N), np.int32), bodies=np.zeros(s.steps, np.int32), ties=np.zeros((s.steps, ctx.N), np.int32),
               count_max=np.zeros(s.steps, np.int32), count_skips=np.zeros(s.steps, np.int32), island_max=np.zeros(s.steps, np.int32))
    if inject:
        run["injections"][0] = s.inj
        assert F.apply_to_oracle(ctx, worlds, run["reset"], s.inj) > 0
    prev = run["reset"]["toievents"]
    for t in range(s.steps):
        for e, w in enumerate(worlds):
            w.toi_counters(reset=True)
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
            c = w.toi_counters()
            run["bodies"][t] += c["bodies"]
            run["ties"][t, e] = c["ties"]
            run["count_skips"][t] += c["count_skips"]
            run["count_max"][t] = max(run["count_max"][t], c["count_max"])
            run["island_max"][t] = max(run["island_max"][t], c["island_max"])
        snap = F.snapshot(ctx, worlds, env)
        for f in F.LANE_FIELDS + F.SLOT_FIELDS:
            assert np.isfinite(snap[f]).all(), "oracle state not finite: %s %s step %d" % (name, f, t + 1)
        run["events"][t] = snap["toievents"] - prev
        prev = snap["toievents"]
        run["steps"].append(snap)
    _RUNS[key] = run
    return run


def reach(run):
    """What a run reaches, from the oracle alone: TOI events, the most events of one creature in one step, the most bodies with an
    event in one step (and that step), the most pairs / touching manifolds on a body, the largest sub-step island, events won on a
    tie, the most events one pair took in one step, visits skipped beyond 8, bodies asleep at injection that were woken."""
    s, ctx = run["scene"], run["ctx"]
    out = dict(creatures=ctx.N, bodies=int(ctx.live.sum()), events=int(run["events"].sum()),
               step_events=int(run["events"].max(initial=0)), queue=int(run["bodies"].max(initial=0)), queue_step=int(np.argmax(run["bodies"])) + 1,
               ties=int(run["ties"].sum()), count_max=int(run["count_max"].max(initial=0)), count_skips=int(run["count_skips"].sum()),
               island=int(run["island_max"].max(initial=0)), pairs=0, touching=0, event_pairs=0, slept=0, woken=0)
    for t, snap in enumerate(run["steps"]):
        pair = F.masks(ctx, snap)["cedge"]
        touch = (pair & (snap["ctouch"] != 0)).sum(axis=0)
        out["pairs"] = max(out["pairs"], int(snap["ccount"].max()))
        out["touching"] = max(out["touching"], int(touch.max()))
        hit = run["events"][t] > 0
        if hit.any():       # the pairs a body with an event holds after that step (the alpha pass walks them all)
            out["event_pairs"] = max(out["event_pairs"], int(snap["ccount"][hit].max()))
    if 0 in run["injections"]:
        asleep = (run["injections"][0]["awake"] == 0) & ctx.live
        out["slept"] = int(asleep.sum())
        out["woken"] = int((asleep & (np.max([st["awake"] for st in run["steps"]], axis=0) != 0)).sum())
    # the creatures lifted out of reach never hold a pair: the scene's host-known bound on the queue is its low bodies
    high = ~s.low
    out["high_pairs"] = int(max(st["ccount"][high].max(initial=0) for st in run["steps"]))
    out["low_bodies"] = int(ctx.live[s.low].sum())
    return out


def queue_bounds(run):
    """-> (lower [steps], upper): the oracle's bodies with a TOI event per step, and the scene's bodies within reach of the ground."""
    return run["bodies"], int(run["ctx"].live[run["scene"].low].sum())


def left_out(run, wide=False):
    """Creatures beyond the build's slots at any step (state_forge.left_out, which looks at N_STEPS snapshots at a time) -> count."""
    gone = np.zeros(run["ctx"].N, bool)
    for c0 in range(0, len(run["steps"]), F.N_STEPS):
        steps = run["steps"][c0:c0 + F.N_STEPS]
        gone |= F.left_out(dict(ctx=run["ctx"], steps=steps), *CAPACITY[wide])[0] < min(F.N_STEPS, len(steps))
    return int(gone.sum())


HEADER = ("| scene | branch | creatures x lanes | steps | TOI events | most in one creature-step | most bodies queued in a step (step) | "
          "most pairs on a body (on a body with an event) | most touching | largest island | events won on a tie | "
          "most events of a pair in a step | asleep at injection / woken |")


def row(name, st, K):
    return "| %s | %s | %d x %d | %d | %d | %d | %d (%d) | %d (%d) | %d | %d | %d | %d | %d / %d |" % (
        name, scene(name).branch, st["creatures"], K, scene(name).steps, st["events"], st["step_events"], st["queue"], st["queue_step"],
        st["pairs"], st["event_pairs"], st["touching"], st["island"], st["ties"], st["count_max"], st["slept"], st["woken"])


if __name__ == "__main__":
    import os
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as O
    O.build()
    print(HEADER)
    for name in (sys.argv[1:] or ALL_SCENES):
        t0 = time.time()
        run = oracle_run(O, name)
        st = reach(run)
        print(row(name, st, run["ctx"].K) + "  left out %d / wide %d, skips %d, queue/step %s (%.1f s)" % (
            left_out(run), left_out(run, True), st["count_skips"], run["bodies"].tolist(), time.time() - t0))
        sys.stdout.flush()
