"""The step kernels on time steps and joint limits no trajectory uses (tests/step_forge.py), on a real MI355X (pytest -m gpu).

Every other GPU parity test steps with (1/50, 180, 60) on joints limited to exactly +-pi/2.  Here the Morphology carries other
limits, torques and controller offsets into `reset`, rem2d_world_step_ex is called with the schedule's dt and iteration counts,
and after EVERY call the whole arena is compared with `==` against the oracle's state after the same steps
(test_injected_state_gpu.mismatches: body columns, joint impulses, motor speed, limit state, every body's pair list in list order,
position iterations, TOI events, reward, done, fitness, wall of death) plus invdt0 == 1.0f / dt.  Every case runs under the five
launch forms of test_tick_split_gpu.FORMS (step train, velocity+post per step, two launches per step, and the 128-lane train and
per-step forms) and the fused step kernel with continuous physics, once with discrete physics, and equal0 / push / alternating in
the wide build.  The `const` schedules make 15 single-step calls and then 4 calls of 5 steps, `alternating` calls of 1 / 2 / 3
steps, budget_mix 25 / 10 / 15: the step train's hand-over runs at every dt.

No creature may carry an error bit the oracle does not justify (only pi/2@const10+kick30 has one creature beyond 24 pair slots,
from the step on at which the oracle shows it), never REM2D_ERR_HANDOVER, and handover_failures() stays 0.

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
import sys

import numpy as np
import pytest

import state_forge as F
import step_forge as S
from test_injected_state_gpu import inject, mismatches, read_state
from test_tick_split_gpu import FORMS as TICK_FORMS

pytestmark = pytest.mark.gpu

CONT = 1
# (tile shape for reset, launch options): test_tick_split_gpu's five (its two_launches_per_step is the two-launch form) + the fused kernel
FORMS = dict(TICK_FORMS, fused_step_kernel=(None, {"pipeline": 0}))


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
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd.world import BatchedWorld
    return BatchedWorld


@pytest.fixture(scope="module")
def tally():
    t = {}
    yield t
    out = sys.__stdout__
    out.write("\nstep-forge parity: case | tests | creature-steps compared | creatures left out\n")
    for name in S.CASES:
        if name in t:
            out.write("  %-24s | %2d | %6d | %d\n" % (name, t[name][0], t[name][1], t[name][2]))
    out.flush()


def run_bucket(gpu, run, terrain, flags, form, wide, schedule=None):
    """-> (creature-steps compared, creatures left out); AssertionError with every difference of the first call that has one."""
    from gym_rem2d_amd import _lib
    ctx, morph, case = run["ctx"], run["ctx"].morph, run["case"]
    schedule = schedule or S.SCHEDULES[case.schedule]
    pair_slots, solver_slots = _lib.capacity(wide)[:2]
    first, bits = S.left_out(run, pair_slots, solver_slots)
    shape, opts = FORMS[form]
    w = gpu(morph.n_envs, morph.lanes, flags, wide=wide, options=opts)
    try:
        w.set_terrain(terrain)
        w.reset(morph, tile_shape=shape)
        assert w.contact_slots == pair_slots
        compared, snap = 0, run["reset"]
        for c, (n, dt, vi, pi) in enumerate(schedule):
            if c in run["injections"]:
                inject(w, ctx, snap, run["injections"][c])
            w.step_ex(n, dt, vi, pi)
            keep = first > c
            snap = run["calls"][c]
            where = "call %d (%d x dt %.9g, %d / %d)" % (c, n, dt, vi, pi)
            st = read_state(w)
            bad = mismatches(ctx, st, snap, keep, pair_slots, where)
            if not (st["invdt0"] == np.float32(1.0) / np.float32(dt)).all():
                bad.append("%s: invdt0 %s" % (where, np.unique(st["invdt0"])))
            err = st["err"]
            if (err[keep] != 0).any():
                bad.append("%s: error bits %s on creatures the oracle does not justify" % (where, err[keep][err[keep] != 0]))
            if (err & F.ERR_HANDOVER).any():
                bad.append("%s: REM2D_ERR_HANDOVER" % where)
            gone = ~keep
            if ((err[gone] & bits[gone]) != bits[gone]).any():
                bad.append("%s: left-out creatures without their capacity bit: err %s, oracle %s" % (where, err[gone], bits[gone]))
            assert not bad, "\n".join(bad)
            compared += n * int(keep.sum())
        assert w.handover_failures() == 0
        return compared, int((first < len(schedule)).sum())
    finally:
        w.close()


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
    compared = gone = 0
    for run in runs:
        a, b = run_bucket(gpu, run, terrain, flags, form, wide)
        compared, gone = compared + a, gone + b
    assert compared > 0
    t = tally.setdefault(name, [0, 0, 0])
    t[0], t[1], t[2] = t[0] + 1, t[1] + compared, t[2] + gone
    print("%s: %d creature-steps compared, %d creatures left out" % (_id(case), compared, gone))
