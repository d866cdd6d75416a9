"""Host half of the TOI-form tests (tests/toi_forge.py): the oracle alone runs every forged scene and each test asserts that the
scene MEETS the condition of the branch it is for -- measured on the oracle (TOI events per creature and step, pairs, touching
manifolds, and rem2d_oracle_toi_counters: sub-step island size, events won on a tie, a pair's events within a step), never on
the kernel -- so that the GPU half (tests/test_toi_forms_gpu.py), which compares the kernels with these very runs, exercises
what its ids say.  A pure host model of the kernel's dealing (toi_forge.lanes_per_body) states for every GPU case the lanes per
body G it guarantees: the scene's bodies within reach of the ground bound the work list from above, the oracle's bodies with
a TOI event in that step from below.

Not met, and said so here and in DESIGN.md section 9 rather than dropped: no scene makes one pair take more than 8 TOI events within
ONE step (b2_maxSubSteps; a pair's count starts again with every step).  The most the oracle shows anywhere -- `repeat`, 9 000
single-body throws into V notches and wedges, the wedging terrains of terrain_forge under 60 m/s kicks -- is 5."""
import numpy as np
import pytest

import replay as R
import state_forge as F
import toi_forge as Z

CASES = Z.gpu_cases()


@pytest.fixture(scope="module")
def twin():
    from oracle import cpu_twin
    cpu_twin.build()

    class World(cpu_twin.CpuWorld):
        """CpuWorld under BatchedWorld's signatures (as in tests/test_replay_host.py)."""
        contact_slots = cpu_twin.CONTACT_SLOTS

        def __init__(self, n_envs, lanes, flags=0, wide=False, options=None):
            super().__init__(n_envs, lanes, flags)

        def reset(self, morph, tile_shape=None):
            super().reset(morph)

        def handover_failures(self):
            return 0
    return World


def _root_kind(run):
    """per creature: 1 box / 2 circle root, and whether it has two bodies"""
    ctx = run["ctx"]
    return ctx.field("shape")[:, 0], ctx.live.sum(axis=1) > 1


@pytest.mark.parametrize("name", Z.ALL_SCENES)
def test_scene_meets_its_condition(oracle, name):
    run = Z.oracle_run(oracle, name)
    s, ctx, st = run["scene"], run["ctx"], Z.reach(run)
    print(Z.row(name, st, ctx.K))
    assert ctx.N % Z.WAVE == 0                                   # padding does not thin the work list
    assert st["events"] > 0 and st["high_pairs"] == 0
    # within the capacity of the build it is compared in; the wide-only scene is beyond the default build's
    assert Z.left_out(run, wide=s.wide_only) == 0
    assert (Z.left_out(run, wide=False) > 0) == s.wide_only
    ev = run["events"].sum(axis=0)
    root, two = _root_kind(run)
    if s.branch in ("ladder", "flags") and name.startswith("ladder"):
        assert run["bodies"][:5].sum() > 0                       # they land within the first steps
        assert (ev[(root == 1) & ~two] > 0).any() and (ev[(root == 2) & ~two] > 0).any()
        assert two.any() == (ctx.K * int(name.split("-")[1][1:]) >= 128) and (not two.any() or (ev[two] > 0).any())
        assert st["bodies"] * Z.WAVE <= int(name.split("-")[1][1:]) * ctx.N * ctx.K         # the body density the id promises
    if s.branch == "crowd":
        assert st["queue"] == st["low_bodies"]                   # every body within reach queues in ONE step
        assert (st["low_bodies"] < st["bodies"]) == (name == "crowd-odd")
    if s.branch == "many pairs":
        assert st["event_pairs"] > 8                             # more pair slots than lanes at the largest G < 64 under test
        assert st["island"] > Z.KR and st["touching"] >= 4       # a sub-step island beyond the constraints kept in registers
        assert (ev[root == 1] > 0).any() and (ev[root == 2] > 0).any()
        assert (st["touching"] > Z.CAPACITY[False][1]) == s.wide_only and st["pairs"] <= Z.CAPACITY[s.wide_only][0]
    if s.branch == "tie":
        ties = run["ties"].sum(axis=0)
        assert (ties[0::2] > 0).any() and (ties[1::2] > 0).any()          # on the joint of two edges, and on the box corner
        n_poly = len(run["profile"].polys)
        last = run["steps"][-1]
        touch = F.masks(ctx, last)["cedge"] & (last["ctouch"] != 0)
        on_box, on_edge = (touch & (last["cedge"] < n_poly)).any(axis=(0, 2)), (touch & (last["cedge"] >= n_poly)).any(axis=(0, 2))
        assert (on_box & on_edge & (ties > 0))[1::2].any()       # a tie between a static box and the edge beside it
        assert not on_box[0::2].any()
    if s.branch == "repeat":
        assert st["step_events"] >= 3 and st["count_max"] >= 3   # several events of one body, and of one PAIR, within one step
        assert st["count_max"] <= 8 and st["count_skips"] == 0   # (the skip beyond 8 is NOT reached: module docstring)
    if s.branch == "flags":
        assert s.flags == Z.CONT | Z.SLEEP_RESET_ALWAYS and st["slept"] > 0
        asleep = (s.inj["awake"] == 0) & ctx.live
        assert (ev[~asleep.any(axis=1)] > 0).any()               # the awake ones have their events
        if name.startswith("sleepers"):                          # a body asleep stays where it is: no pair, no event
            assert st["woken"] == 0 and not ev[asleep.any(axis=1)].any()


def test_every_gpu_scene_is_proven_here():
    assert {c.scene for c in CASES} == set(Z.ALL_SCENES)
    assert len({Z.case_id(c) for c in CASES}) == len(CASES)


def test_lanes_per_body_model():
    """toi_heavy_body's arithmetic on known values: per = max(h, ceil(queued / blocks)), G the largest power of two with G * per <= 64."""
    assert Z.lanes_per_body(1, 4096, 1) == (1, 64) and Z.lanes_per_body(1, 4096, 64) == (1, 64) and Z.lanes_per_body(1, 4096, 65) == (2, 32)
    assert Z.lanes_per_body(3, 4096, 1) == (3, 16) and Z.lanes_per_body(64, 128, 1) == (64, 1)
    assert [Z.lanes_per_body(1, 64, q)[1] for q in (8, 9, 16, 17, 32, 33, 64)] == [8, 4, 4, 2, 2, 1, 1]
    for h in (1, 2, 5, 64):
        g = [Z.lanes_per_body(h, 1024, q)[1] for q in range(1, 1025)]
        assert all(a >= b for a, b in zip(g, g[1:])) and g[0] == Z.lanes_per_body(h, 1024, 1)[1]
    assert Z.guaranteed_G(1, 256, 33, 64) == 4 and Z.guaranteed_G(1, 256, 32, 64) is None and Z.guaranteed_G(1, 256, 0, 64) is None


@pytest.mark.parametrize("case", [c for c in CASES if c.G is not None], ids=Z.case_id)
def test_gpu_case_guarantees_its_G(oracle, case):
    """By option: every launch that queues anything takes the id's G (the bodies within reach cannot push `per` beyond
    heavy_per_wave).  By queue length (default options): in the step in which the oracle shows the most bodies with an event, the
    bounds leave one G, the id's."""
    run = Z.oracle_run(oracle, case.scene)
    lower, upper = Z.queue_bounds(run)
    Lp = run["ctx"].N * run["ctx"].K
    assert lower.max() > 0 and lower.max() <= upper
    if case.heavy is not None:
        assert case.G * case.heavy == Z.WAVE
        assert Z.guaranteed_G(case.heavy, Lp, 1, upper) == case.G
    else:
        t = int(np.argmax(lower))
        assert Z.guaranteed_G(1, Lp, int(lower[t]), upper) == case.G
        assert case.G in (4, 2, 1)


def test_crowd_odd_takes_the_three_exits(oracle):
    """131 bodies over 16 blocks: per = 9, G = 4 -- `slot >= per` in every wavefront, `idx >= queued` in block 14, `block * per >=
    queued` in block 15 (toi_heavy_body), and the bounds meet: the queue's length is known, not only its G."""
    run = Z.oracle_run(oracle, "crowd-odd")
    lower, upper = Z.queue_bounds(run)
    queued, blocks = int(lower.max()), run["ctx"].N * run["ctx"].K // Z.WAVE
    assert queued == upper == 131 and blocks == 16
    per, g = Z.lanes_per_body(1, blocks * Z.WAVE, queued)
    assert (per, g) == (9, 4) and queued % per != 0
    slots = Z.WAVE // g
    assert slots > per                                                                   # slot >= per
    assert [b for b in range(blocks) if b * per >= queued] == [15]                       # block * per >= queued
    assert any(b * per < queued <= b * per + s for b in range(blocks) for s in range(per))   # idx >= queued within a started block


TWIN_SCENES = Z.LADDER_SCENES[:1] + Z.LADDER_SCENES[-2:] + ["crowd-G4", "crowd-G1", "manypairs-K2", "tie-K4", "repeat-K8", "sleepers-K2",
                                                           Z.ladder_name(64, sleep=True)]


@pytest.mark.parametrize("name", TWIN_SCENES)
def test_twin_replays_the_scene(twin, oracle, name):
    """The GPU half's call of replay.replay on the oracle-backed twin of the ABI.  The twin keeps its state in oracle worlds, so a
    write to its arena is no injection (tests/test_replay_host.py): it replays the scene's UN-injected run, from the same reset."""
    run = Z.oracle_run(oracle, name, inject=False)
    ctx, s = run["ctx"], run["scene"]
    got = R.replay(lambda: R.make_world(twin, ctx.morph, run["profile"], s.flags, "velpost", False), ctx, run["reset"],
                   [1] * s.steps, run["steps"], 24)
    assert got == (s.steps * ctx.N, 0)


def test_injection_is_what_makes_the_scene(oracle):
    """Self-check: without its injection a scene misses its branch within its steps -- nothing lands in the crowd and tie scenes,
    no body of `repeat` has a second event in a step -- so the conditions asserted above are not met by any run."""
    for name in ("crowd-G1", "tie-K2"):
        assert Z.reach(Z.oracle_run(oracle, name, inject=False))["events"] == 0
    st = Z.reach(Z.oracle_run(oracle, "repeat-K2", inject=False))
    assert st["step_events"] < 3 and st["count_max"] < 3
