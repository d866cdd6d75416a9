"""Small populations that drive the 2-point block solve (csrc/rem2d_solver.h: contact_solve, contact_solve_pair, contact_solve_quad)
through all four of its cases, shared by tests/test_block_solver_host.py (oracle alone) and tests/test_block_solver_gpu.py.

After case 1 of the block solve the kernels ask, with one ballot over the lanes in the 2-point branch, whether any of them still needs
cases 2 .. 4 and branch around the three when none does.  Each population below is ONE velocity tile (64 lanes) that reaches one code
path of the step train's velocity body by the count of touching manifolds NC it holds when a step starts:

| population | tile                                   | path                                                              |
|------------|----------------------------------------|-------------------------------------------------------------------|
| pair       | four creatures in 16 lanes each        | NC <= 32: two lanes per manifold, contact_solve_pair              |
| classic    | 20 two-box chains (lane bucket 2)      | 32 < NC <= 64: one lane per manifold, contact_solve               |
| spilled    | 32 two-box chains (lane bucket 2)      | NC > 64: manifolds of rank >= 64 through scratch (v4_contact_spilled) |
| toi        | the `pair` creatures, thrown down      | TOI events: the TOI solve's contact_solve_quad, besides the above |

Protocol, state_forge's: settle, then N_STEPS steps with injections (binary32 values, the same bits on both sides) before some of
them, the oracle's whole visible state recorded after every step.  The injection `tumble` gives one creature in eight an upward
velocity of 0.1 - 0.4 m/s (its manifolds of the step before are solved while the body leaves: case 4; it is back on the ground a few
steps later), two in eight a spin per body (one point of a lying box lifts: cases 2 and 3) and leaves the rest alone (case 1), so that
the tile keeps the count of manifolds that holds it on its path.  The steps before the first injection find the chains at rest.

Coverage (`coverage`) is read from the oracle's own output: a manifold that is touching with two points when a step starts and is
found again after the step on the same body with the same edge and the same two feature keys shows the accumulated normal impulses of
the step's LAST velocity iteration: both > 0 case 1, n1 == 0 < n0 case 2, n0 == 0 < n1 case 3, both 0 case 4 -- a proxy, and enough
to show that the fallback code ran.  Manifolds whose solver constraint falls back to one point (b2ContactSolver's condition-number
test, k11^2 >= 1000 det K) do not enter the block solve: the test is restated in binary64 from the pose and the manifold before the
step, and a manifold within a factor 2 of the threshold is not counted at all.  A tile-step is `skipped` if it has such manifolds and
every one of them shows case 1, `fallback` if one shows another case, `mixed` if the tile also holds a touching 1-point manifold.
"""
import numpy as np

import state_forge as F

CONT = 1
N_STEPS = 15
K_MAX_CONDITION = 1000.0

# name -> (seed of the injections' generator, chosen so that the ORACLE ALONE meets test_block_solver_host.py's conditions; settle steps;
# steps before which `tumble` is injected; throw: lift and throw down first (TOI events))
POPS = {
    "pair": dict(seed=4, settle=75, inject=(3, 7, 11), throw=False),
    "classic": dict(seed=0, settle=75, inject=(3, 7, 11), throw=False),
    "spilled": dict(seed=2, settle=75, inject=(3, 7, 11), throw=False),
    "toi": dict(seed=2, settle=75, inject=(0, 7, 11), throw=True),
}
# the count of touching manifolds of the tile at the start of a step that puts it on the population's path
NC_RANGE = {"pair": (1, 32), "classic": (33, 64), "spilled": (65, 10 ** 9), "toi": (1, 64)}

_POPS = {}


def _shifted(morph, x0, dx):
    """creature e moved x0 + e dx along the track (binary32 sums, before either side sees the morphology): off the flat start pad,
    every creature on its own piece of the rough ground"""
    a, K = morph.arrays, morph.lanes
    for e in range(morph.n_envs):
        sl = slice(e * K, (e + 1) * K)
        live = a["shape"][sl] != 0
        a["x"][sl][live] = (a["x"][sl][live] + np.float32(x0 + e * dx)).astype(np.float32)
    return morph


def population(name):
    """name -> (terrain, Morphology of one 64-lane tile).  The creatures are boxes 0.5 x 0.8 m: one alone, and chains of two on the
    `left` / `top` site with a controller of amplitude 0 (they lie still once settled: every manifold in case 1) or 0.5."""
    if name in _POPS:
        return _POPS[name]
    from gym_rem2d_amd import make_terrain, synthetic
    from gym_rem2d_amd.compiler import Morphology
    box = synthetic.spec_from_tree(synthetic.chain_tree(1))
    quiet = synthetic.spec_from_tree(synthetic.chain_tree(2, "left", amp=0.0))
    quiet_top = synthetic.spec_from_tree(synthetic.chain_tree(2, "top", amp=0.0))
    moving = synthetic.spec_from_tree(synthetic.chain_tree(2, "left"))
    if name in ("pair", "toi"):
        morph = _shifted(Morphology.from_specs([box, quiet, moving, quiet_top], 16), 2.0, 1.3)
    elif name == "classic":
        morph = _shifted(Morphology.from_specs([quiet] * 20, 2), 2.0, 0.37)
    elif name == "spilled":
        morph = _shifted(Morphology.from_specs([quiet] * 32, 2), 2.0, 0.53)
    else:
        raise KeyError(name)
    assert morph.n_envs * morph.lanes <= 64 and len(tiles(morph)) == 1
    _POPS[name] = (make_terrain(4), morph)
    return _POPS[name]


def tiles(morph):
    """[(first creature, end)] of the velocity tiles as the library cuts them."""
    from gym_rem2d_amd import _lib
    n, k = morph.n_envs, morph.lanes
    cpb = max(1, 64 // k)
    t = _lib.plan_tiles(morph.arrays["parent"], morph.arrays["jround"], n, k, (n + cpb - 1) // cpb * cpb)
    return [(int(a), min(int(b), n)) for a, b in zip(t[:-1], t[1:]) if a < n]


def tumble(name, ctx, snap, rng):
    """{field: array}: per creature one of (lift off: 1 in 8, spin every body: 2 in 8, nothing)."""
    N, K = ctx.N, ctx.K
    kind = rng.permutation(N) % 8
    vx, vy, w = snap["vx"].copy(), snap["vy"].copy(), snap["w"].copy()
    up = F._f32(rng.uniform(0.1, 0.4, (N, 1)) * np.ones((1, K)))
    spin = F._f32(rng.normal(0.0, 3.0, (N, K)))
    vy[kind == 0] = up[kind == 0]
    w[(kind == 1) | (kind == 2)] = spin[(kind == 1) | (kind == 2)]
    return dict(vx=vx, vy=vy, w=w, awake=np.ones((N, K), np.int32))


def throw(ctx, snap):
    """lifted 1.5 m and thrown down at 20 m/s: the bodies cross the ground within a step (TOI events)."""
    N, K = ctx.N, ctx.K
    return dict(py=F._f32(snap["py"].astype(np.float64) + 1.5), vx=np.zeros((N, K), np.float32),
                vy=np.full((N, K), -20.0, np.float32), w=np.zeros((N, K), np.float32), awake=np.ones((N, K), np.int32))


def _two_point_records(ctx, worlds, snap):
    """The touching manifolds the coming step solves, from the oracle's state before it: (touching per lane [N, K], records of the
    2-point ones: (creature, lane, index among the body's touching manifolds, edge, key0, key1, conditioning k11^2 / (1000 det K)))."""
    touch = np.zeros((ctx.N, ctx.K), np.int64)
    recs = []
    one_point = np.zeros((ctx.N, ctx.K), np.int64)
    for e, w in enumerate(worlds):
        mass = w.mass()
        for bi, lane in enumerate(ctx.slots[e]):
            t = 0
            for k in range(int(snap["ccount"][e, lane])):
                if not snap["ctouch"][k, e, lane]:
                    continue
                if snap["cnpt"][k, e, lane] == 2:
                    m = w.manifold(bi, k).astype(np.float64)
                    c = np.array([snap["px"][e, lane], snap["py"][e, lane]], np.float64)
                    a = float(snap["ang"][e, lane])
                    rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
                    if snap["ctype"][k, e, lane] == 1:       # e_faceA: the static shape's face; points in the body's frame
                        normal = m[0:2]
                        pts = [c + rot @ m[4:6], c + rot @ m[6:8]]
                    else:                                        # e_faceB: the body's face; points in the static (world) frame
                        normal = rot @ m[0:2]
                        pts = [m[4:6], m[6:8]]
                    rn = [float((p - c)[0] * normal[1] - (p - c)[1] * normal[0]) for p in pts]
                    im, ii = float(mass[bi, 0]), float(mass[bi, 1])
                    k11, k22, k12 = im + ii * rn[0] ** 2, im + ii * rn[1] ** 2, im + ii * rn[0] * rn[1]
                    det = k11 * k22 - k12 * k12
                    cond = k11 * k11 / (K_MAX_CONDITION * det) if det > 0.0 else np.inf
                    recs.append((e, int(lane), t, int(snap["cedge"][k, e, lane]), int(snap["ckey0"][k, e, lane]),
                                 int(snap["ckey1"][k, e, lane]), cond))
                else:
                    one_point[e, lane] += 1
                t += 1
            touch[e, lane] = t
    return touch, one_point, recs


def _case_after(snap, rec):
    """The pattern (1 .. 4) the manifold of `rec` shows after the step, None if it is not found again with both its points."""
    e, lane, _, edge, k0, k1, _ = rec
    for k in range(int(snap["ccount"][e, lane])):
        if (snap["cedge"][k, e, lane] == edge and snap["cnpt"][k, e, lane] == 2 and snap["ckey0"][k, e, lane] == k0
                and snap["ckey1"][k, e, lane] == k1):
            n0, n1 = float(snap["cn0"][k, e, lane]), float(snap["cn1"][k, e, lane])
            if n0 > 0.0 and n1 > 0.0:
                return 1
            if n1 == 0.0 and n0 > 0.0:
                return 2
            if n0 == 0.0 and n1 > 0.0:
                return 3
            if n0 == 0.0 and n1 == 0.0:
                return 4
            return None
    return None


_RUNS = {}


def oracle_run(O, name):
    """-> dict(ctx, settled, injections {step: {field: array}}, steps [snapshot after step 1 .. N_STEPS], before [(touching [N, K],
    1-point touching [N, K], 2-point records) of the state each step starts from, injection applied])."""
    if name in _RUNS:
        return _RUNS[name]
    cfg = POPS[name]
    terrain, morph = population(name)
    ctx = F.Ctx(morph, name)
    ot = F.oracle_terrain(O, terrain)
    md = morph.as_dict()
    worlds = [O.World.from_morph(ot, md, e, CONT) for e in range(ctx.N)]
    env = dict(reward=np.zeros(ctx.N, np.float32), done=np.zeros(ctx.N, np.int32), everdone=np.zeros(ctx.N, np.int32),
               fitness=np.zeros(ctx.N, np.float64), frozen=np.zeros(ctx.N, np.int32), steps=np.zeros(ctx.N, np.int32))

    def step():
        for e, w in enumerate(worlds):
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

    for _ in range(cfg["settle"]):
        step()
    rng = np.random.default_rng([cfg["seed"], 20262])
    run = dict(ctx=ctx, name=name, settled=F.snapshot(ctx, worlds, env), injections={}, steps=[], before=[])
    snap = run["settled"]
    for t in range(N_STEPS):
        if t in cfg["inject"]:
            inj = throw(ctx, snap) if cfg["throw"] and t == 0 else tumble(name, ctx, snap, rng)
            run["injections"][t] = inj
            F.apply_to_oracle(ctx, worlds, snap, inj)
            snap = F.snapshot(ctx, worlds, env)
        run["before"].append(_two_point_records(ctx, worlds, snap))
        step()
        snap = F.snapshot(ctx, worlds, env)
        for f in F.LANE_FIELDS + F.SLOT_FIELDS:
            assert np.isfinite(snap[f]).all(), "oracle state not finite: %s %s step %d" % (name, f, t + 1)
        run["steps"].append(snap)
    _RUNS[name] = run
    return run


def ranks(touch, c0, c1):
    """rank of manifold t of the body on (creature e, lane) in the tile's contact map: (t, lane of the tile) order (vel4_body)."""
    flat = touch[c0:c1].reshape(-1)
    K = touch.shape[1]

    def rank(e, lane, t):
        pos = (e - c0) * K + lane
        return int(sum((flat > tt).sum() for tt in range(t)) + (flat[:pos] > t).sum())
    return rank


def coverage(run):
    """Over the tile-steps on the population's path (NC_RANGE): how often each pattern shows, the tile-steps skipped / fallback / mixed,
    and the patterns of the manifolds of rank >= 64 (the spilled path's)."""
    ctx, name = run["ctx"], run["name"]
    lo, hi = NC_RANGE[name]
    out = dict(cases={1: 0, 2: 0, 3: 0, 4: 0}, spilled_cases={1: 0, 2: 0, 3: 0, 4: 0}, skipped=0, fallback=0, mixed=0, tile_steps=0,
               on_path=0, nc=[], unseen=0, one_point=0, two_point=0)
    for t, (touch, one_point, recs) in enumerate(run["before"]):
        for c0, c1 in tiles(ctx.morph):
            nc = int(touch[c0:c1].sum())
            out["tile_steps"] += 1
            out["nc"].append(nc)
            if not lo <= nc <= hi:
                continue
            out["on_path"] += 1
            rank = ranks(touch, c0, c1)
            seen, block = [], 0
            for r in recs:
                if not c0 <= r[0] < c1 or r[6] >= 1.0:     # (falls back to one point: not in the block solve)
                    continue
                block += 1
                if r[6] > 0.5:                             # (too near the threshold for a binary64 restatement to say)
                    continue
                case = _case_after(run["steps"][t], r)
                if case is None:
                    out["unseen"] += 1
                    continue
                seen.append(case)
                out["cases"][case] += 1
                if rank(r[0], r[1], r[2]) >= 64:
                    out["spilled_cases"][case] += 1
            out["two_point"] += block
            out["one_point"] += int(one_point[c0:c1].sum())
            if block and len(seen) == block and all(c == 1 for c in seen):
                out["skipped"] += 1
            if any(c != 1 for c in seen):
                out["fallback"] += 1
            if block and one_point[c0:c1].sum() > 0:
                out["mixed"] += 1
    return out


if __name__ == "__main__":
    import os
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as O
    O.build()
    for name in POPS:
        t0 = time.time()
        run = oracle_run(O, name)
        cov = coverage(run)
        toi = int((run["steps"][-1]["toievents"] - run["settled"]["toievents"]).sum())
        gone = int((F.left_out(run)[0] < N_STEPS).sum())
        print(name, {k: v for k, v in cov.items() if k != "nc"}, "NC", cov["nc"], "TOI", toi, "left out", gone, "(%.1f s)" % (time.time() - t0))
