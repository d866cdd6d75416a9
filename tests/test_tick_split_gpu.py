"""The ramp / steady split of the velocity tiles' tick loop (csrc/rem2d_vel4.h, vel4_body) against the oracle, bit for bit.

A tile runs its period groups [base, base + P) on the general code while base < tLo or base + P > tHi and on the steady body in
between, where tLo = the latest first tick of any of its joints and manifolds and tHi = the earliest first tick + iters * P.
Every case below is one or two 64-lane blocks that cross one boundary of that split, stepped through the step train, the per-step
launches (velocity + position in one launch and in two) and the 128-lane train, and compared with the oracle (`np.array_equal` on
the eight body columns) three steps after reset -- the creatures spawn 2 m up and are still airborne -- and again
after they have landed and settled.

What a case claims to hit is asserted through a host-side restatement: `tile_split` is the loop's split, `tile_plan` the kernel's
contact plan (vel4_body's `plan` lambda and its P / P + 1 choice: every body's contact tick, every creature's rotation, the sub-slots
per phase), fed with the real tile table (`rem2d_plan_tiles_shape`) and with the touching manifolds per body that the oracle holds one
step before the compared one: those are the manifolds that step solves.  From them follow the period a tile takes, the first tick of
every joint and manifold, hence tLo / tHi and the count of steady groups, exactly.  `no_steady_group_possible` is a bound that holds
whatever the contacts do.
"""
import functools

import numpy as np
import pytest

from conftest import oracle_terrain
from replay import LAUNCH_FORMS, TICK_FORMS, need_gpu

CONT = 1   # REM2D_FLAG_CONTINUOUS == oracle.FLAG_CONTINUOUS
FORMS = {name: LAUNCH_FORMS[form] for name, form in TICK_FORMS.items()}      # id -> (tile shape for reset, launch options)


# ---------------- host-side restatement of the split ----------------
def tile_split(firsts, period, iters):
    """(tLo, tHi, steady period groups) of a tile whose constraints first fire at ticks `firsts` (vel4_body's loop, restated)."""
    t_lo, t_hi = max(firsts), min(firsts) + iters * period
    n_ticks = max(firsts) + (iters - 1) * period + 1
    return t_lo, t_hi, sum(1 for base in range(0, n_ticks, period) if base >= t_lo and base + period <= t_hi)


def tile_table(morph, lanes_per_tile):
    """[(first creature, end)] of the velocity tiles as the library cuts them (rem2d_plan_tiles_shape: 64-lane tiles, or shape 1's
    128-lane ones; at most 32 creatures to a tile)."""
    from gym_rem2d_amd import _lib
    n, k = morph.n_envs, morph.lanes
    cpb = max(1, 64 // k)
    t = _lib.plan_tiles(morph.arrays["parent"], morph.arrays["jround"], n, k, (n + cpb - 1) // cpb * cpb,
                        tile_shape=1 if lanes_per_tile == 128 else -1)
    return [(int(a), min(int(b), n)) for a, b in zip(t[:-1], t[1:]) if a < n]


def tiles_of(morph, lanes_per_tile):
    """[(joint rounds, period)] of the tiles."""
    n, k = morph.n_envs, morph.lanes
    sched = morph.arrays["jround"].reshape(n, k)
    parent = morph.arrays["parent"].reshape(n, k)
    out = []
    for c0, c1 in tile_table(morph, lanes_per_tile):
        s, p = sched[c0:c1], parent[c0:c1]
        rounds = (s & 0xff)[p >= 0]
        if rounds.size:
            out.append((rounds.tolist(), int(((s >> 16) & 0xff).max())))
    return out


# csrc/rem2d_vel4.h, the DEFAULT build: the wide build unrolls for 5 phases, so a period-4 tile may take 5 there and the plans asserted
# below do not hold for it.  The period a tile takes is inferred from this restatement, not read back from the kernel.
V4_PHASES, V4_PLUS1_GAIN = 4, 2


def creature_plan(rounds, parent, n_touch, pc):
    """vel4_body's plan(Pc) for one awake creature: (tick of iteration 0 of every body's manifolds, rotation included; the rotation).
    A body's window runs from its last joint round to its first + Pc - 1; greedily, the phase inside the windows of the most
    unplaced touching bodies takes them (ties: the later phase); the creature is rotated so that its phase with the most
    manifolds on one body (ties: the first) becomes phase 0."""
    n = len(rounds)
    first, last = [10 ** 9] * n, [-1] * n
    for b in range(n):
        if parent[b] >= 0:
            for x in (b, parent[b]):
                first[x], last[x] = min(first[x], rounds[b]), max(last[x], rounds[b])
    wlo = [last[b] if last[b] >= 0 else 0 for b in range(n)]
    wlen = [first[b] + pc - last[b] if last[b] >= 0 else pc for b in range(n)]
    off, placed = list(wlo), [n_touch[b] == 0 for b in range(n)]

    def dist(s, b):
        return (s - wlo[b] % pc) % pc
    for _ in range(min(pc, V4_PHASES)):
        cover = [sum(1 for b in range(n) if not placed[b] and s < pc and dist(s, b) < wlen[b]) for s in range(V4_PHASES)]
        cstar = 0
        for s in range(1, V4_PHASES):
            if s < pc and cover[s] >= cover[cstar]:
                cstar = s
        for b in range(n):
            if not placed[b] and cover[cstar] > 0 and dist(cstar, b) < wlen[b]:
                off[b], placed[b] = wlo[b] + dist(cstar, b), True
    heavy, heavy_phase = 0, 0
    for s in range(min(pc, V4_PHASES)):
        most = max([n_touch[b] for b in range(n) if off[b] % pc == s] + [0])
        if most > heavy:
            heavy, heavy_phase = most, s
    delta = (pc - heavy_phase) % pc if heavy > 0 else 0
    return [o + delta for o in off], delta


def tile_plan(creatures, period):
    """creatures: [(joint rounds per body, parent per body, touching manifolds per body)] of a tile of the flexible shapes ->
    (the period it takes, first ticks of all its joints and manifolds, contact sub-slots per phase)."""
    def plan(pc):
        subs, firsts = [0] * V4_PHASES, []
        for rounds, parent, n_touch in creatures:
            off, delta = creature_plan(rounds, parent, n_touch, pc)
            for b in range(len(rounds)):
                if parent[b] >= 0:
                    firsts.append(rounds[b] + delta)
                if n_touch[b] > 0:
                    firsts.append(off[b])
                    subs[off[b] % pc] = max(subs[off[b] % pc], n_touch[b])
        return subs, firsts
    subs, firsts = plan(period)
    if period < V4_PHASES and sum(subs) >= 3:
        subs_q, firsts_q = plan(period + 1)
        if sum(subs_q) + V4_PLUS1_GAIN <= sum(subs):
            return period + 1, firsts_q, subs_q
    return period, firsts, subs


def planned_tiles(morph, touch, lanes_per_tile):
    """tile_plan of every tile of a population whose bodies hold `touch` [n_envs, lanes] touching manifolds."""
    n, k = morph.n_envs, morph.lanes
    sched = morph.arrays["jround"].reshape(n, k)
    parent = morph.arrays["parent"].reshape(n, k)
    nb = np.asarray(morph.n_bodies)
    out = []
    for c0, c1 in tile_table(morph, lanes_per_tile):
        cr = [((sched[e, :nb[e]] & 0xff).tolist(), parent[e, :nb[e]].tolist(), touch[e, :nb[e]].tolist()) for e in range(c0, c1)]
        period = int(((sched[c0:c1] >> 16) & 0xff).max())
        out.append((period,) + tile_plan(cr, period))
    return out


def no_steady_group_possible(rounds, period, iters):
    """True if tLo >= tHi whatever the contacts do: tLo >= the last round; tHi <= first round + (P' - 1) + iters P', P' = P + 1."""
    return max(rounds) >= min(rounds) + period + (iters * (period + 1))


def test_restatement_names_the_boundaries():
    """No GPU: the populations below really sit where the cases say (chain8: joint rounds 0 .. 6 at period 2)."""
    from gym_rem2d_amd import synthetic
    (rounds, period), = tiles_of(synthetic.chain_population(8, 8, "top"), 64)
    assert (sorted(set(rounds)), period) == ([0, 1, 2, 3, 4, 5, 6], 2)
    assert [tile_split(rounds, period, it) for it in (1, 3, 4, 5, 180)] == [(6, 2, 0), (6, 6, 0), (6, 8, 1), (6, 10, 2), (6, 360, 177)]
    assert no_steady_group_possible(rounds, period, 1) and not no_steady_group_possible(rounds, period, 4)
    for name, pop in _populations().items():
        for lanes in (64, 128):
            for rounds, period in tiles_of(pop, lanes):
                assert tile_split(rounds, period, 180)[2] >= 170, name
    assert tile_table(_populations()["chain2_left"], 128) == [(0, 32), (32, 64)]   # (32 creatures to a tile at the most)
    # the contact plan worked by hand on a four-body chain (joint rounds 2, 1, 0 from the root's child on: period 2) with two manifolds
    # on each of the two middle bodies.  At period 2 their windows are one tick each, of different phases: 2 + 2 sub-slots.  At
    # period 3 the windows are ticks 2-3 and 1-2: both bodies run in tick 2, the creature is rotated by one tick (phase 2 -> 0): 2.
    chain = ([0, 2, 1, 0], [-1, 0, 1, 2])
    assert creature_plan(chain[0], chain[1], [0, 2, 2, 0], 2) == ([2, 2, 1, 0], 0)
    assert creature_plan(chain[0], chain[1], [0, 2, 2, 0], 3) == ([3, 3, 3, 1], 1)
    assert tile_plan([chain + ([0, 2, 2, 0],)], 2) == (3, [3, 3, 2, 3, 1], [2, 0, 0, 0])
    assert tile_plan([chain + ([0, 1, 1, 0],)], 2) == (2, [2, 2, 1, 1, 0], [1, 1, 0, 0])   # (too few sub-slots to pay a tick)


@functools.lru_cache(maxsize=None)
def _populations():
    from gym_rem2d_amd import synthetic
    from gym_rem2d_amd.compiler import Morphology
    ls = [s for s in synthetic.lsystem_specs(range(48), mutate_odd=True) if s.n_bodies <= 16]
    period = ((Morphology.from_specs(ls, 16).arrays["jround"].reshape(len(ls), 16) >> 16) & 0xff).max(1)
    mix = [ls[i] for p in (4, 3, 2) for i in np.nonzero(period == p)[0][:4]]   # (from_specs keeps the order of its specs)
    return {
        "chain4_top": synthetic.chain_population(32, 4, "top"),      # period 2; two 64-lane blocks = one 128-lane tile
        "chain4_left": synthetic.chain_population(32, 4, "left"),
        "chain2_left": synthetic.chain_population(64, 2, "left"),    # lands flat: > 64 manifolds per tile, three on one body
        "chain8_top": synthetic.chain_population(8, 8, "top"),       # joint rounds 0 .. 6 at period 2: the few-iterations cases
        "lsystem_mix": Morphology.from_specs(mix, 16),               # three blocks of periods 4, 3 and 2; bodies with 3-4 manifolds
        # eight copies of one period-3 creature whose contacts of steps 76-78 make a tile take the period 4 (two 64-lane tiles, one of 128)
        "lsystem_plus1": Morphology.from_specs(synthetic.lsystem_specs([110], mutate_odd=True) * 8, 16),
    }


SETTLED = {"chain4_top": 45, "chain4_left": 40, "chain2_left": 75, "chain8_top": 40, "lsystem_mix": 45, "lsystem_plus1": 78}
_REFS = {}


def _reference(oracle, terrain, name, vel_iters=180):
    """Oracle run of a population: bodies + reward after 3 and after SETTLED steps, touching manifolds per body before steps 3 and SETTLED."""
    key = (name, vel_iters)
    if key not in _REFS:
        morph = _populations()[name]
        ot = oracle_terrain(oracle, terrain)
        d, nb = morph.as_dict(), np.asarray(morph.n_bodies)
        worlds = [oracle.World.from_morph(ot, d, e, CONT) for e in range(morph.n_envs)]

        def snap():
            bodies = np.zeros((morph.n_envs, morph.lanes, 8), dtype=np.float32)
            for e, w in enumerate(worlds):
                bodies[e, :nb[e]] = w.bodies()
            return bodies

        def touching():
            cnt = np.zeros((morph.n_envs, morph.lanes), dtype=np.int64)
            for e, w in enumerate(worlds):
                for b in range(int(nb[e])):
                    c, _ = w.contacts(b)
                    cnt[e, b] = int((c[:, 3] != 0).sum()) if len(c) else 0
            return cnt

        out, T = {}, SETTLED[name]
        for step in range(1, T + 1):
            if step in (3, T):
                out["touch", step] = touching()
            for w in worlds:
                w.env_step_ex(1.0 / 50, vel_iters, 60)
            if step in (3, T):
                out["bodies", step] = snap()
        _REFS[key] = out
    return _REFS[key]


@pytest.fixture(scope="module")
def gpu():
    return need_gpu(world=True)


def _compare(gpu, oracle, terrain, name, form, vel_iters=180):
    morph = _populations()[name]
    nb = np.asarray(morph.n_bodies)
    ref = _reference(oracle, terrain, name, vel_iters)
    shape, opts = FORMS[form]
    w = gpu(morph.n_envs, morph.lanes, CONT, options=opts)
    w.set_terrain(terrain)
    w.reset(morph, tile_shape=shape)
    done = 0
    for T in (3, SETTLED[name]):
        w.step_ex(T - done, 1.0 / 50, vel_iters, 60)
        done = T
        got = w.bodies()
        for e in range(morph.n_envs):
            assert np.array_equal(got[e, :nb[e]], ref["bodies", T][e, :nb[e]]), (name, form, vel_iters, T, e)
    assert int(w.view("err").max()) == 0
    w.close()
    return ref


def _tile_sums(cnt, morph, lanes_per_tile):
    return [int(cnt[c0:c1].sum()) for c0, c1 in tile_table(morph, lanes_per_tile)]


# ---------------- the cases ----------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["step_train", "velpost_per_step", "train_128_lanes"])
@pytest.mark.parametrize("vel_iters,steady", [(1, 0), (3, 0), (4, 1), (5, 2)])
def test_few_velocity_iterations(gpu, oracle, rough_terrain, vel_iters, steady, form):
    """(a) rem2d_world_step_ex's vel_iters: 1 and 3 leave no steady group (tLo = 6 >= tHi = 2, 6), 4 exactly one, 5 two -- exact
    while the chains are airborne (step 3); with 1 iteration no steady group is possible after landing either."""
    ref = _compare(gpu, oracle, rough_terrain, "chain8_top", form, vel_iters)
    assert ref["touch", 3].sum() == 0 and ref["touch", SETTLED["chain8_top"]].sum() > 0
    (rounds, period), = tiles_of(_populations()["chain8_top"], 64)
    assert tile_split(rounds, period, vel_iters)[2] == steady
    if vel_iters == 1:
        assert no_steady_group_possible(rounds, period, vel_iters)


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["chain4_top", "chain4_left", "lsystem_mix"])
def test_periods_and_contact_phases(gpu, oracle, rough_terrain, name, form):
    """(b), (c), (e), (f): periods 2 (the chains) and 2, 3, 4 (the L-system mix) through every form; airborne creatures without a
    manifold at step 3.  Landed, by the restated plan: every tile keeps its manifolds in registers and runs > 160 steady groups; every
    chain tile has a phase with a contact sub-slot and a phase without one; a tile of the mix runs three sub-slots in one phase (three
    manifolds on one body) and holds a creature without any manifold."""
    ref = _compare(gpu, oracle, rough_terrain, name, form)
    morph = _populations()[name]
    T = SETTLED[name]
    touch = ref["touch", T]
    assert ref["touch", 3].sum() == 0 and touch.sum() > 0
    lanes = 128 if FORMS[form][0] == 1 else 64
    assert max(_tile_sums(touch, morph, lanes)) <= 64                     # (registers hold them all)
    plans = planned_tiles(morph, touch, lanes)
    for period, taken, firsts, subs in plans:
        assert tile_split(firsts, taken, 180)[2] > 160
    if name.startswith("chain4"):
        assert all(taken == 2 and min(subs[:2]) == 0 and max(subs[:2]) > 0 for _, taken, _, subs in plans), plans
    else:
        assert sorted({taken for _, taken, _, _ in plans}) == ([2, 4] if lanes == 128 else [2, 3, 4])   # (the 128-lane tiles: periods 4 + 3 together, then 2)
        assert any(max(subs) >= 3 for _, _, _, subs in plans)
        assert ((touch > 0).sum(1) == 0).any()                            # (f) a creature without any manifold beside landed ones


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_tile_takes_one_more_phase(gpu, oracle, rough_terrain, form):
    """(b) V4_PLUS1_GAIN: by the restated plan every tile of these period-3 creatures runs the step compared (and the two before it)
    at period 4 -- sub-slots 2 instead of 4 -- with its manifolds in registers and its steady groups at that period."""
    ref = _compare(gpu, oracle, rough_terrain, "lsystem_plus1", form)
    morph = _populations()["lsystem_plus1"]
    lanes = 128 if FORMS[form][0] == 1 else 64
    touch = ref["touch", SETTLED["lsystem_plus1"]]
    assert max(_tile_sums(touch, morph, lanes)) <= 64
    plans = planned_tiles(morph, touch, lanes)
    assert len(plans) == (1 if lanes == 128 else 2)
    for period, taken, firsts, subs in plans:
        assert (period, taken) == (3, 4) and sum(subs) >= 2
        assert tile_split(firsts, taken, 180)[2] > 160


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["step_train", "velpost_per_step", "train_128_lanes"])
def test_tile_that_spills_manifolds(gpu, oracle, rough_terrain, form):
    """(d) two-module chains lying flat, 32 to a tile in either shape: 96 touching manifolds per tile against 64 in registers, up to
    three on one body: its steady groups read the manifolds beyond the registers from scratch, gated by the key's phase and sub-slot."""
    ref = _compare(gpu, oracle, rough_terrain, "chain2_left", form)
    morph = _populations()["chain2_left"]
    cnt = ref["touch", SETTLED["chain2_left"]]
    sums = _tile_sums(cnt, morph, 128 if FORMS[form][0] == 1 else 64)
    assert len(sums) == 2 and min(sums) > 64 and cnt.max() >= 3
    for period, taken, firsts, subs in planned_tiles(morph, cnt, 128 if FORMS[form][0] == 1 else 64):
        assert tile_split(firsts, taken, 180)[2] > 160 and max(subs) >= 3
