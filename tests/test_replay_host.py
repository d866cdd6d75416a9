"""tests/replay.py without a GPU: the replay loop, the comparison and the error-bit verdict that deliver the verdict of every GPU
parity suite, driven on the oracle-backed twin of the ABI (oracle/cpu_twin.py CpuWorld) instead of a BatchedWorld.

The twin keeps its state in oracle worlds and only exports it to its arena, so a write to the arena is NOT an injection: nothing
here injects, and the protocols pass on un-injected runs only -- the natural runs of the injected-state protocol (two worlds,
marks), a terrain run and a step-forge schedule (step_ex, invdt0).  The negative controls are what this module is for: a
difference forged into the oracle's snapshots, or reported by an adapter, must come back as an AssertionError that names it, and a
difference outside a field's mask must not.
"""
import copy

import numpy as np
import pytest

import replay as R
import state_forge as F
import step_forge as S
import terrain_forge as G

CONT = 1
MARKS = (5, 10, F.N_STEPS)      # the marks of a three-injection scenario


@pytest.fixture(scope="module")
def twin():
    from oracle import cpu_twin
    cpu_twin.build()

    class World(cpu_twin.CpuWorld):
        """CpuWorld under BatchedWorld's signatures: one build (24 pair slots), one launch form, no step train to fail a hand-over.
        `err`: what the adapter claims after every call (the twin does not maintain the field)."""
        contact_slots, err, failures = cpu_twin.CONTACT_SLOTS, 0, 0

        def __init__(self, n_envs, lanes, flags=0, wide=False, options=None):
            super().__init__(n_envs, lanes, flags)

        def reset(self, morph, tile_shape=None):
            super().reset(morph)

        def step(self, n_steps=1):
            super().step(n_steps)
            self.view("err")[0] = self.err

        def handover_failures(self):
            return self.failures
    return World


def natural(twin, run, steps=None, marks=MARKS, first=None, bits=None, World=None):
    """The injected-state protocol (test_injected_state_gpu.run_bucket) on an un-injected run."""
    ctx = run["ctx"]
    terrain, _ = F.population("lsystem")
    return R.replay(lambda: R.make_world(World or twin, ctx.morph, terrain, CONT, "step_train", False), ctx, run["settled"],
                    [1] * F.N_STEPS, steps or run["steps"], 24, settle=F.SETTLE, first=first, bits=bits, marks=marks)


@pytest.fixture(scope="module")
def run2(oracle):
    run = F.oracle_run(oracle, "lsystem", 0, None, CONT)
    assert run["ctx"].K == 2
    return run


@pytest.mark.parametrize("bucket,lanes", [(0, 2), (3, 16)])
def test_injected_state_protocol(twin, oracle, bucket, lanes):
    run = F.oracle_run(oracle, "lsystem", bucket, None, CONT)
    assert run["ctx"].K == lanes
    assert natural(twin, run) == (F.N_STEPS * run["ctx"].N, 0)


def test_terrain_protocol(twin, oracle):
    """test_terrain_gpu.run_bucket's call: from reset, marks 1 / 10 / 60.  49 320 creature-steps over saw's 7 ids, 3 of them
    other populations' at 15 000 in all: 8 580 for an L-system id."""
    compared = 0
    for run in G.runs_of(oracle, "saw", "lsystem", CONT):
        ctx = run["ctx"]
        compared += R.replay(lambda: R.make_world(twin, ctx.morph, run["profile"], CONT, "step_train", False), ctx, run["reset"],
                             [1] * G.N_STEPS, run["steps"], 24, marks=(1, 10, G.N_STEPS))[0]
    assert compared == G.N_STEPS * 143 == 8580


def test_step_forge_protocol(twin, oracle):
    """test_step_forge_gpu.run_bucket's call: one world, step_ex, invdt0.  20 160 creature-steps over alternating's 7 ids: 2 880."""
    case = S.CASES["pi/2@alternating"]
    terrain, _ = S.case_morphs(case)
    compared = 0
    for run in S.case_runs(oracle, case, CONT):
        ctx = run["ctx"]
        first, bits = S.left_out(run)
        c, gone = R.replay(lambda: R.make_world(twin, ctx.morph, terrain, CONT, "per_step_128_lanes", False), ctx, run["reset"],
                           S.SCHEDULES[case.schedule], run["calls"], 24, first=first, bits=bits, check=R.invdt0)
        assert gone == 0
        compared += c
    assert compared == 2880


def forged(run, step, field, at, value=None):
    """run["steps"] with ONE entry of snapshot `step` (1-based) changed: to `value`, or by one ulp."""
    steps = copy.deepcopy(run["steps"])
    a = steps[step - 1][field]
    a[at] = np.nextafter(a[at], np.float32(np.inf)) if value is None else value
    assert a[at] != run["steps"][step - 1][field][at]
    return steps


def test_one_ulp_is_reported_from_both_worlds(twin, run2):
    with pytest.raises(AssertionError) as e:        # step 8 is no mark: the single-step world alone sees the snapshot
        natural(twin, run2, forged(run2, 8, "px", (0, 0)))
    assert "single step 8 px: 1 differ, first at (0, 0)" in str(e.value) and "multi" not in str(e.value)
    with pytest.raises(AssertionError) as e:        # step 10 is a mark
        natural(twin, run2, forged(run2, 10, "px", (0, 0)))
    assert "single step 10 px: 1 differ" in str(e.value) and "multi step 10 px: 1 differ" in str(e.value)
    assert "step 11" not in str(e.value)            # the first call that differs, and no later one


def test_slot_field_under_its_mask_is_reported(twin, run2):
    step, snap = next((t + 1, s) for t, s in enumerate(run2["steps"]) if F.masks(run2["ctx"], s)["ckey0"].any())
    at = tuple(int(x[0]) for x in np.nonzero(F.masks(run2["ctx"], snap)["ckey0"]))
    with pytest.raises(AssertionError, match=r"single step %d ckey0: 1 differ, first at \(%d, %d, %d\)" % ((step,) + at)):
        natural(twin, run2, forged(run2, step, "ckey0", at, snap["ckey0"][at] + 1))


def test_outside_the_mask_is_not_reported(twin, run2):
    """A dead lane, and a pair row beyond ccount: the masks are part of the contract."""
    ctx = run2["ctx"]
    dead = tuple(int(x[0]) for x in np.nonzero(~ctx.live))
    steps = forged(run2, 8, "px", dead, np.float32(123.0))
    row = int(steps[7]["ccount"][0, 0])
    steps[7]["cn0"][row, 0, 0] = np.float32(7.0)
    steps[7]["cedge"][row, 0, 0] = 99
    assert natural(twin, run2, steps) == (F.N_STEPS * ctx.N, 0)


def test_left_out_creature_without_its_bit(twin, run2):
    """first / bits forged: the oracle would justify leaving creature 0 out from step 4 on, and the world shows no bit."""
    n = run2["ctx"].N
    first, bits = np.full(n, F.N_STEPS, np.int32), np.zeros(n, np.int32)
    first[0], bits[0] = 3, F.ERR_PAIR
    with pytest.raises(AssertionError, match="single step 4: left-out creatures without their"):
        natural(twin, run2, first=first, bits=bits)
    # the same creature carrying its bit from that step on passes, and is counted out

    class Late(twin):
        singles = 0

        def step(self, n_steps=1):
            self.singles += n_steps == 1
            self.err = F.ERR_PAIR if self.singles > 3 else 0
            super().step(n_steps)
    assert natural(twin, run2, first=first, bits=bits, marks=(), World=Late) == (F.N_STEPS * n - (F.N_STEPS - 3), 1)


@pytest.mark.parametrize("err,text", [(F.ERR_PAIR, r"single step 1: error bits \[1\] on creatures the oracle"),
                                      (F.ERR_HANDOVER, "single step 1: REM2D_ERR_HANDOVER")], ids=["pair", "handover"])
def test_error_bit_on_a_kept_creature(twin, run2, err, text):
    class World(twin):
        def step(self, n_steps=1):
            self.err = 0 if n_steps == F.SETTLE else err        # (clean while settling: the start state has its own check)
            super().step(n_steps)
    with pytest.raises(AssertionError, match=text):
        natural(twin, run2, World=World)


def test_error_bit_at_the_start(twin, run2):
    class World(twin):
        err = F.ERR_SOLVER
    with pytest.raises(AssertionError):
        natural(twin, run2, World=World)


def test_failed_hand_over_is_reported(twin, run2):
    class World(twin):
        failures = 1
    with pytest.raises(AssertionError, match=r"single world: handover_failures\(\) 1"):
        natural(twin, run2, World=World)
