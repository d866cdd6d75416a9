"""The step kernels on injected states the trajectories never reach (tests/state_forge.py), on a real MI355X (pytest -m gpu).

Every other parity test starts from `reset`; here both sides settle 25 steps, are shown to be equal, receive the SAME binary32
values -- the GPU through ``BatchedWorld.view(name)``: the arena is the whole state between two steps (rem2d_world_adopt's
contract), the oracle through set_body_state / set_joint_impulses / set_contact_impulses -- and are compared with `==` after
each of 15 further single-step launches, and in a second world given the same injections after every ``step(n)`` launch that
runs up to the next injection (the step train's own hand-over).  The loop and what it compares: tests/replay.py.

A creature leaves the comparison only from the step on at which the ORACLE shows a body beyond the build's pair or solver
slots (state_forge.left_out, capped at 2 % of a population by the host half); its REM2D_F_ERR must then carry that capacity
bit, never the hand-over bit, and any error bit on another creature fails the test (replay.verdict).

What it found: the `impulses` scenario failed in every launch form alike (e.g. L-system bucket 2, creature 5, one step after
normal impulses were scaled by -1: ct0 gpu 6.7318475e-09 / oracle 1.086219e-06).  The friction constraint clamped with the
median of (a, -m, m), m = friction * normalImpulse, which is b2Clamp only for m >= 0; csrc/rem2d_math.h fclamp_sym is the
fix, test_negative_normal_impulse_friction_clamp the reduced case.  No trajectory from `reset` reaches a negative normal
impulse (the solver leaves none), an adopted arena can.

Measured on an MI355X: 150 ids in about 30 s, all passing; per scenario 24 525 creature-steps compared on the single-step worlds
over its 15 ids (limit 3 000 over 5; kick150 34 257 over 21 ids with 11 creatures left out, each carrying its capacity bit).
"""
import copy

import numpy as np
import pytest

import replay as R
import state_forge as F

pytestmark = pytest.mark.gpu

CONT = 1
FORMS = ("step_train", "velpost", "two_launches", "fused_step_kernel")     # this module's ids are replay.LAUNCH_FORMS' own names


def _cases():
    out = []
    for sc in F.SCENARIOS:
        for pop in F.populations_of(sc):
            for form in FORMS:                       # continuous physics through every launch form
                out.append((sc, pop, form, CONT, False))
            out.append((sc, pop, "step_train", 0, False))   # b2World.continuousPhysics off
    for pop in F.populations_of("kick150"):          # the wide build shares the source: 32 pair / 12 solver slots, nobody left out
        out.append(("kick150", pop, "step_train", CONT, True))
        out.append(("kick150", pop, "velpost", 0, True))
    return out


def _id(c):
    return "%s-%s-%s-%s%s" % (c[0], c[1], c[2], "continuous" if c[3] else "discrete", "-wide" if c[4] else "")


@pytest.fixture(scope="module")
def gpu():
    return R.need_gpu(world=True)


@pytest.fixture(scope="module")
def tally():
    yield from R.tally("injected-state parity (single-step worlds): scenario", F.SCENARIOS)


def run_bucket(gpu, run, terrain, flags, form, wide):
    """-> (creature-steps compared on the single-step world, creatures left out), through replay.replay: both worlds settle, the
    second one runs in one launch from injection to injection."""
    from gym_rem2d_amd import _lib
    ctx = run["ctx"]
    pair_slots, solver_slots = _lib.capacity(wide)[:2]
    first, bits = F.left_out(run, pair_slots, solver_slots)
    return R.replay(lambda: R.make_world(gpu, ctx.morph, terrain, flags, form, wide), ctx, run["settled"], [1] * F.N_STEPS,
                    run["steps"], pair_slots, settle=F.SETTLE, injections=run["injections"], first=first, bits=bits,
                    marks=sorted(run["injections"]) + [F.N_STEPS])


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_injected_state_bit_exact(gpu, oracle, tally, case):
    scenario, pop, form, flags, wide = case
    from gym_rem2d_amd import _lib
    assert _lib.FLAG_CONTINUOUS == oracle.FLAG_CONTINUOUS == CONT
    terrain, _ = F.population(pop)
    runs = F.population_runs(oracle, pop, scenario, flags)   # the oracle first: a non-finite state never reaches the GPU
    pair_slots, solver_slots = _lib.capacity(wide)[:2]
    F.check_left_out_cap(scenario, runs, pair_slots, solver_slots)
    compared, gone = map(sum, zip(*[run_bucket(gpu, run, terrain, flags, form, wide) for run in runs]))
    assert compared > 0
    R.count(tally, scenario, _id(case), compared, gone)


@pytest.mark.parametrize("form", list(FORMS))
def test_negative_normal_impulse_friction_clamp(gpu, oracle, form):
    """Regression, reduced from `impulses`: two-lane L-system creatures standing on the rough terrain, every normal impulse
    negated (tangent impulses, joints and bodies untouched).  The friction constraint of the next step's first velocity
    iteration then clamps to [-m, m] with m = friction * normalImpulse < 0, for which b2Clamp returns -m; a median of the
    three (the kernels' fclamp, right for lo <= hi) returned something else and the tangent impulse of e.g. creature 5 came out
    6.7e-09 where the oracle has 1.086e-06 -- in every formulation alike.  The kernels use fclamp_sym there now."""
    terrain, _ = F.population("lsystem")
    run = F.oracle_run(oracle, "lsystem", 0, "impulses", CONT, make=F.negative_normal_injection)
    assert run["ctx"].K == 2 and run["changed"] > 0
    # (the creatures touch down during the compared steps: the injections at steps 5 and 10 are the ones that find impulses)
    assert min(float(inj[f].min()) for inj in run["injections"].values() for f in ("cn0", "cn1")) < 0.0
    compared, gone = run_bucket(gpu, run, terrain, CONT, form, False)
    assert compared == F.N_STEPS * run["ctx"].N and gone == 0


def test_replay_notices_one_ulp(gpu, oracle):
    """The runner on the real arena: the lane-2 bucket of the natural L-system run under the step train passes against the oracle's
    snapshots and fails against a copy in which one word (px of creature 0 after step 8) is moved by one ulp."""
    terrain, _ = F.population("lsystem")
    run = F.oracle_run(oracle, "lsystem", 0, None, CONT)
    assert run["ctx"].K == 2 and not run["injections"]
    assert run_bucket(gpu, run, terrain, CONT, "step_train", False) == (F.N_STEPS * run["ctx"].N, 0)
    steps = copy.deepcopy(run["steps"])
    steps[7]["px"][0, 0] = np.nextafter(steps[7]["px"][0, 0], np.float32(np.inf))
    with pytest.raises(AssertionError, match="single step 8 px: 1 differ"):
        run_bucket(gpu, dict(run, steps=steps), terrain, CONT, "step_train", False)
