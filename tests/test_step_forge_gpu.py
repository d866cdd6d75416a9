"""The step kernels on time steps and joint limits no trajectory uses (tests/step_forge.py), on a real MI355X (pytest -m gpu).

Every other GPU parity test steps with (1/50, 180, 60) on joints limited to exactly +-pi/2.  Here the Morphology carries other
limits, torques and controller offsets into `reset`, rem2d_world_step_ex is called with the schedule's dt and iteration counts,
and after EVERY call the whole arena is compared with `==` against the oracle's state after the same steps (replay.replay: every
field the oracle exposes) plus invdt0 == 1.0f / dt.  Every case runs under the five launch forms of replay.TICK_FORMS (step train,
velocity+post per step, two launches per step, and the 128-lane train and per-step forms) and the fused step kernel with continuous
physics, once with discrete physics, and equal0 / push / alternating in the wide build.  The `const` schedules make 15 single-step
calls and then 4 calls of 5 steps, `alternating` calls of 1 / 2 / 3 steps, budget_mix 25 / 10 / 15: the step train's hand-over runs
at every dt.

No creature may carry an error bit without the oracle's own state showing why (replay.verdict; only pi/2@const10+kick30 has one
creature beyond 24 pair slots, from the step on at which the oracle shows it), never the hand-over bit, and handover_failures()
stays 0.

dt itself: rem2d_world_step_ex refuses a dt that is not finite or not > 0 (tests/test_abi.py, include/rem2d.h) -- b2World::Step's
dt == 0 (collide only) has no path in the kernels, which guard only invDt0 and the TOI scan with h > 0.

What it found: nothing.  All 164 ids pass; no kernel was changed.  The LIM_EQUAL branches, the dtRatio warm start, h * torque, the
clamps, the sleep timer and the TOI sweeps agree with the oracle bit for bit at every dt and limit tried.  That the cases would
notice: with the LIM_EQUAL branch of the velocity limit solve taken out of a scratch copy of the oracle, equal0@const50 differs
from call 12 - 17 on (when the creatures land; every bucket), equal_off@const50 from 15 - 17, equal_edge@const50 from call 0 and
equal0@alternating from call 5 - 13, so every id of those cases fails; with `motorImpulse *= dtRatio` taken out, every bucket of
pi/2@alternating, push@alternating and pi/2@budget_mix differs at call 1, the first change of dt, and so do all their ids.

Measured on an MI355X: 164 ids in about 20 s, each under 0.6 s after the first; per case 19 600 creature-steps compared over its 7
ids (alternating 20 160, budget_mix 28 000, the -pairs cases 4 900, 2 800 more per wide id); pi/2@const10+kick30 19 468 with one
creature left out in each of its six continuous ids, carrying its pair-overflow bit.
"""
import pytest

import replay as R
import step_forge as S

pytestmark = pytest.mark.gpu

CONT = 1
FORMS = dict(R.TICK_FORMS, fused_step_kernel="fused_step_kernel")     # this module's id -> replay.LAUNCH_FORMS name


def _cases():
    out = []
    for name in S.CASES:
        for form in FORMS:
            out.append((name, form, CONT, False))
        out.append((name, "step_train", 0, False))
    for name in S.WIDE_CASES:
        out.append((name, "step_train", CONT, True))
    return out


def _id(c):
    return "%s-%s-%s%s" % (c[0], c[1], "continuous" if c[2] else "discrete", "-wide" if c[3] else "")


@pytest.fixture(scope="module")
def gpu():
    return R.need_gpu(world=True)


@pytest.fixture(scope="module")
def tally():
    yield from R.tally("step-forge parity: case", S.CASES)


def run_bucket(gpu, run, terrain, flags, form, wide):
    """-> (creature-steps compared: n per kept creature and call of n steps, creatures left out), through replay.replay: ONE world
    from reset, the schedule's step_ex calls, invdt0 == 1.0f / dt after each."""
    from gym_rem2d_amd import _lib
    ctx = run["ctx"]
    pair_slots, solver_slots = _lib.capacity(wide)[:2]
    first, bits = S.left_out(run, pair_slots, solver_slots)
    return R.replay(lambda: R.make_world(gpu, ctx.morph, terrain, flags, FORMS[form], wide), ctx, run["reset"],
                    S.SCHEDULES[run["case"].schedule], run["calls"], pair_slots, injections=run["injections"], first=first,
                    bits=bits, check=R.invdt0)


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_step_forge_bit_exact(gpu, oracle, tally, case):
    name, form, flags, wide = case
    from gym_rem2d_amd import _lib
    assert _lib.FLAG_CONTINUOUS == oracle.FLAG_CONTINUOUS == CONT
    c = S.CASES[name]
    terrain, _ = S.case_morphs(c)
    runs = S.case_runs(oracle, c, flags)         # the oracle first: a non-finite state never reaches the GPU
    pair_slots, solver_slots = _lib.capacity(wide)[:2]
    n = sum(r["ctx"].N for r in runs)
    assert S.n_left_out(runs, pair_slots, solver_slots) <= (int(S.LEFT_OUT_CAP * n) if c.kicks else 0)
    compared, gone = map(sum, zip(*[run_bucket(gpu, run, terrain, flags, form, wide) for run in runs]))
    assert compared > 0
    R.count(tally, name, _id(case), compared, gone)
