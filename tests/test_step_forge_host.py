"""Host half of the step-argument / joint-parameter tests (tests/step_forge.py): the oracle alone runs every case and the tests
assert that the case REACHES the code it is for; the GPU half (tests/test_step_forge_gpu.py) compares the kernels with these
very runs.

What the cases reach, continuous physics, 80 L-system creatures (20 two-body ones in the -pairs cases), every step of the run
(`python tests/step_forge.py` prints this, and the discrete-physics table):

| case                   | steps | joint-steps inactive / lower / upper / equal | limit-state changes | at a limit with motor impulse | max motor impulse | 60-iteration steps | body-steps asleep | TOI sub-steps | top speed | most pairs | left out |
|------------------------|----|----------------------------|------|-------|-------|------|-----|------|------|----|---|
| equal0@const50         | 35 | 0 / 0 / 0 / 15435          | 0    | 0     | 0     | 541  | 0   | 216  | 8.9  | 5  | 0 |
| equal_off@const50      | 35 | 0 / 0 / 0 / 15435          | 0    | 0     | 0     | 619  | 0   | 206  | 7.4  | 5  | 0 |
| equal_edge@const50     | 35 | 746 / 5092 / 4557 / 5040   | 901  | 9649  | 1     | 1181 | 0   | 213  | 11.8 | 5  | 0 |
| narrow@const50         | 35 | 1441 / 7196 / 6798 / 0     | 1372 | 13994 | 1     | 1060 | 0   | 181  | 15.5 | 5  | 0 |
| above@const50          | 35 | 1357 / 7653 / 6425 / 0     | 1417 | 14078 | 1     | 1149 | 0   | 170  | 15.0 | 5  | 0 |
| below@const50          | 35 | 1372 / 6755 / 7308 / 0     | 1373 | 14063 | 1     | 999  | 0   | 179  | 16.2 | 5  | 0 |
| reversed@const50       | 35 | 0 / 10188 / 5247 / 0       | 9795 | 15435 | 1     | 2093 | 0   | 297  | 14.2 | 6  | 0 |
| wide@const50           | 35 | 15435 / 0 / 0 / 0          | 0    | 0     | 1     | 0    | 0   | 123  | 16.2 | 5  | 0 |
| torque0@const50        | 35 | 7865 / 3932 / 3638 / 0     | 529  | 0     | 0     | 347  | 0   | 185  | 7.1  | 5  | 0 |
| torque_big@const50     | 35 | 12475 / 1342 / 1618 / 0    | 508  | 2960  | 68.4  | 238  | 0   | 110  | 25.2 | 5  | 0 |
| push@const50           | 35 | 8099 / 3783 / 3553 / 0     | 1052 | 7336  | 1     | 902  | 0   | 122  | 19.4 | 5  | 0 |
| equal_edge@const50-pairs | 35 | 15 / 276 / 199 / 210     | 30   | 475   | 1     | 46   | 0   | 28   | 5.8  | 4  | 0 |
| above@const50-pairs    | 35 | 27 / 428 / 245 / 0         | 30   | 673   | 1     | 104  | 0   | 27   | 5.8  | 4  | 0 |
| pi/2@const60           | 35 | 12622 / 1332 / 1481 / 0    | 436  | 2813  | 0.833 | 145  | 0   | 86   | 15.6 | 5  | 0 |
| pi/2@const30           | 35 | 11721 / 1569 / 2145 / 0    | 700  | 3714  | 1.67  | 399  | 44  | 243  | 18.0 | 6  | 0 |
| pi/2@const200          | 35 | 12715 / 1338 / 1382 / 0    | 332  | 2720  | 0.25  | 8    | 0   | 0    | 17.1 | 0  | 0 |
| pi/2@const10           | 35 | 10320 / 2119 / 2996 / 0    | 1640 | 5115  | 5     | 891  | 339 | 1004 | 20.0 | 10 | 0 |
| pi/2@alternating       | 36 | 12722 / 1448 / 1706 / 0    | 522  | 3154  | 2     | 285  | 0   | 139  | 17.8 | 6  | 0 |
| pi/2@budget_mix        | 50 | 17053 / 2157 / 2840 / 0    | 674  | 4997  | 1     | 109  | 0   | 281  | 16.2 | 6  | 0 |
| pi/2@const10+kick30    | 35 | 11184 / 1728 / 2523 / 0    | 1920 | 4251  | 5     | 986  | 29  | 902  | 20.0 | 26 | 1 |
| equal0@alternating     | 36 | 0 / 0 / 0 / 15876          | 0    | 0     | 0     | 546  | 0   | 222  | 9.7  | 5  | 0 |
| above@alternating      | 36 | 1487 / 7843 / 6546 / 0     | 1685 | 14389 | 2     | 1263 | 0   | 195  | 18.4 | 6  | 0 |
| push@alternating       | 36 | 7458 / 4287 / 4131 / 0     | 1197 | 8418  | 2     | 1040 | 0   | 128  | 20.3 | 6  | 0 |

(max motor impulse = h x torque: 1 at 1/50 with the modules' 50 N m, 5 at 1/10, 0.25 at 1/200.  Top speed 20.0 m/s in the const10
cases IS the translation clamp, 2 m / 0.1 s.  One oracle run of a case takes 0.5 - 1 s.)

equal_edge: the issue that asked for these tests expected LIM_EQUAL on the two lower rungs (T - 1 ulp and T, T = 2.0f *
b2_angularSlop).  The test is `fabs(upper - lower) < 2.0f * b2_angularSlop`, strict, and doubling is exact, so upper = T is the
first value that is NOT equal: the oracle shows LIM_EQUAL on the bottom rung only (5040 of 15435 joint-steps) and that is what
is asserted here -- the rungs still sit on both sides of the comparison, one ulp apart.

Who checks the oracle here: its binary64 build (tests/test_oracle_f64.py), with that file's point-wise tolerances (1e-4 in x, y,
angle at every step, 2e-3 in the velocities) and no other.  On that file's own point-wise population (six-module chains in free
flight: joints, limits and motors, no contact) over the WHOLE schedule: equal0@const50 2.2e-5 / 2.4e-6 (pose / velocity, 35
steps), above@const50 6.5e-5 / 7.9e-4, pi/2@alternating 2.4e-5 / 4.5e-5 and equal0@alternating 2.9e-5 / 9.5e-7 (36 steps).  On
the L-system creatures of the cases themselves, which stand on the rough terrain and take TOI sub-steps from the first step:
equal0@const50 holds for 20 steps (2.2e-5 / 4.2e-5); above@const50 holds for 3 steps (1.2e-5 / 2.2e-5) and shows 1.5e-4 in step 4,
where limit states start to flip; pi/2@alternating does not hold for one step (4e-2: 76 of 521 bodies, whole creatures whose
joints reach +-pi/2 in the first step -- the natural trajectories' own first step at 1/50, which test_oracle_f64 compares as a
distribution for that reason), so its point-wise leg is the free-flight one.
"""
import numpy as np
import pytest

import state_forge as F
import step_forge as S

CONT = 1


def _runs(oracle, name, flags=CONT):
    return S.case_runs(oracle, S.CASES[name], flags)


def _limit_states(runs):
    """-> [steps, jointed lanes of all buckets] limit state."""
    return np.concatenate([np.stack([s["jlimit"][r["ctx"].jointed] for s in r["every"]]) for r in runs], axis=1)


def test_the_issue_cases_are_all_there():
    names = set(S.CASES)
    assert {"%s@const50" % v for v in S.VARIANTS if v != "pi/2"} <= names and len(S.VARIANTS) == 12
    assert {"pi/2@%s" % s for s in ("const60", "const30", "const200", "const10", "alternating", "budget_mix")} <= names
    assert {"%s@alternating" % v for v in ("equal0", "above", "push")} <= names and "pi/2@const10+kick30" in names
    for m in S.case_morphs(S.CASES["equal0@const50"])[1]:
        assert m.n_envs <= S.PER_BUCKET
    assert [m.lanes for m in S.case_morphs(S.CASES["equal0@const50"])[1]] == [2, 4, 8, 16]
    for name, sched in S.SCHEDULES.items():
        assert 30 <= sum(c[0] for c in sched) <= (50 if name == "budget_mix" else 40), name
    dts = [c[1] for c in S.SCHEDULES["alternating"]]
    ratios = {round(b / a, 3) for a, b in zip(dts, dts[1:])}
    assert {0.5, 2.0, 4.0, 0.125} <= ratios and {c[0] for c in S.SCHEDULES["alternating"]} == {1, 2, 3}


def test_variants_write_what_they_say(oracle):
    """The joint parameters as the reset kernel and World.from_morph receive them, to the bit."""
    for v, (lo, up) in {"equal0": (0.0, 0.0), "equal_off": (0.3, 0.3), "narrow": (-0.05, 0.05), "above": (0.1, 0.2),
                        "below": (-0.2, -0.1), "reversed": (0.5, -0.5), "wide": (-4.0, 4.0)}.items():
        for m in S.case_morphs(S.CASES[v + "@const50"])[1]:
            j = S.Ctx(m).jointed.reshape(-1)
            assert (m.arrays["lower"][j] == np.float32(lo)).all() and (m.arrays["upper"][j] == np.float32(up)).all(), v
    T = S.EQUAL_T
    assert T == np.float32(2.0) * (np.float32(2.0) / np.float32(180.0) * np.float32(3.14159265359)) and 0.0698 < T < 0.06982
    assert S.EDGE_RUNGS[0] < T == S.EDGE_RUNGS[1] < S.EDGE_RUNGS[2] and S.EDGE_RUNGS[2] - S.EDGE_RUNGS[0] < 2e-8
    for name in ("equal_edge@const50", "equal_edge@const50-pairs"):
        for m in S.case_morphs(S.CASES[name])[1]:
            ctx = S.Ctx(m)
            up, rung = ctx.field("upper")[ctx.jointed], S.edge_rung(ctx)[ctx.jointed]
            assert (ctx.field("lower")[ctx.jointed] == 0).all()
            assert all((up[rung == k] == S.EDGE_RUNGS[k]).all() and (rung == k).any() for k in range(3))
    base = S.case_morphs(S.CASES["pi/2@const60"])[1]
    for v in ("torque0", "torque_big", "push"):
        for m, b in zip(S.case_morphs(S.CASES[v + "@const50"])[1], base):
            j = S.Ctx(m).jointed.reshape(-1)
            assert np.array_equal(m.arrays["lower"], b.arrays["lower"]) and (np.abs(b.arrays["lower"][j]) == np.float32(np.pi / 2)).all()
            if v == "push":
                assert (m.arrays["amp"][j] == 0).all() and set(m.arrays["offset"][j].tolist()) == {3.0, -3.0}
            else:
                assert (m.arrays["torque"][j] == np.float32(0.0 if v == "torque0" else 1e6)).all()
    assert (base[0].arrays["torque"] != 0).any()         # (the shared morphologies are copies: the base is untouched)


@pytest.mark.parametrize("name", ["equal0@const50", "equal_off@const50", "equal0@alternating"])
def test_equal_limits_on_every_joint(oracle, name):
    lim = _limit_states(_runs(oracle, name))
    assert lim.size > 10000 and (lim == S.LIM_EQUAL).all()
    assert (_limit_states(_runs(oracle, name, 0)) == S.LIM_EQUAL).all()


@pytest.mark.parametrize("name", ["equal_edge@const50", "equal_edge@const50-pairs"])
def test_equal_edge_rungs_sit_on_both_sides(oracle, name):
    """T - 1 ulp: LIM_EQUAL on every joint at every step; T and T + 1 ulp: never (the comparison is strict, see the module text)."""
    for r in _runs(oracle, name):
        ctx = r["ctx"]
        rung = S.edge_rung(ctx)
        for s in r["every"]:
            assert (s["jlimit"][ctx.jointed & (rung == 0)] == S.LIM_EQUAL).all()
            assert (s["jlimit"][ctx.jointed & (rung >= 1)] != S.LIM_EQUAL).all()
        assert (ctx.jointed & (rung == 0)).any() and (ctx.jointed & (rung == 1)).any() and (ctx.jointed & (rung == 2)).any()


@pytest.mark.parametrize("name", ["above@const50", "below@const50", "narrow@const50", "above@alternating", "above@const50-pairs"])
def test_narrow_ranges_reach_both_limits_and_change_state(oracle, name):
    lim = _limit_states(_runs(oracle, name))
    assert (lim == S.LIM_AT_LOWER).any() and (lim == S.LIM_AT_UPPER).any() and (lim == S.LIM_INACTIVE).any()
    assert not (lim == S.LIM_EQUAL).any()
    changes = lim[1:] != lim[:-1]
    assert changes.sum() >= 20
    pairs = set(zip(lim[:-1][changes].tolist(), lim[1:][changes].tolist()))
    assert {(0, 1), (1, 0), (0, 2), (2, 0)} <= pairs                   # into and out of either limit


def test_reversed_limits_take_the_if_chain_order(oracle):
    """lower = 0.5 > upper = -0.5: `angle <= lower` is asked first, so a joint is AT_LOWER below 0.5 and AT_UPPER above; never free."""
    lim = _limit_states(_runs(oracle, "reversed@const50"))
    assert set(np.unique(lim).tolist()) == {S.LIM_AT_LOWER, S.LIM_AT_UPPER}


def test_wide_limits_are_never_reached_and_angles_pass_pi(oracle):
    runs = _runs(oracle, "wide@const50")
    assert (_limit_states(runs) == S.LIM_INACTIVE).all()
    top = 0.0
    for r in runs:
        ctx = r["ctx"]
        for s in r["every"]:
            a = s["ang"].astype(np.float64)
            rel = a - np.take_along_axis(a, np.maximum(ctx.parent, 0), axis=1)
            top = max(top, float(np.abs(rel[ctx.jointed] - (ctx.field("angle") - np.take_along_axis(
                ctx.field("angle"), np.maximum(ctx.parent, 0), axis=1)).astype(np.float64)[ctx.jointed]).max()))
    assert np.pi / 2 < top < 4.0     # beyond what +-pi/2 allows (measured: see below) and inside the limit
    print("wide: largest joint angle %.3f" % top)


@pytest.mark.parametrize("name", ["push@const50", "push@alternating"])
def test_push_holds_joints_at_a_limit_with_the_motor_on(oracle, name):
    st = S.reach(_runs(oracle, name))
    base = S.reach(_runs(oracle, "pi/2@const60"))
    assert st["limit_and_motor"] > 5000 and st["limit_and_motor"] > 2 * base["limit_and_motor"]
    # ... for many steps in a row: some joint is at a limit with a motor impulse over the last 20 steps without a break
    held = False
    for r in _runs(oracle, name):
        j = r["ctx"].jointed
        run = np.stack([((s["jlimit"][j] == 1) | (s["jlimit"][j] == 2)) & (s["jmotorimp"][j] != 0) for s in r["every"][-20:]])
        held = held or bool(run.all(axis=0).any())
    assert held


def test_dead_and_strong_motors(oracle):
    for flags in (CONT, 0):
        for r in _runs(oracle, "torque0@const50", flags):
            for s in r["every"]:
                assert (s["jmotorimp"][r["ctx"].jointed] == 0).all()
    assert S.reach(_runs(oracle, "torque_big@const50"))["motor_max"] > 20.0     # far beyond h * 50 N m = 1
    for name, h in (("pi/2@const60", 1 / 60), ("pi/2@const30", 1 / 30), ("pi/2@const200", 1 / 200), ("pi/2@const10", 0.1)):
        top = S.reach(_runs(oracle, name))["motor_max"]      # maxMotorImpulse = h * torque is met, and never passed
        assert top == np.float32(np.float32(h) * np.float32(50.0)), (name, top)


def test_equal_off_uses_all_position_iterations(oracle):
    runs = _runs(oracle, "equal_off@const50")
    assert any((s["positers"] == 60).any() for r in runs for s in r["every"])
    # the start pose violates the limit by 0.3 rad > b2_maxAngularCorrection (8 deg = 0.14): the first iterations of the first step
    # clamp, and every jointed creature needs more than one
    for r in runs:
        assert (r["every"][0]["positers"][r["ctx"].jointed.any(axis=1)] >= 3).all()


def test_alternating_changes_dt_with_live_impulses(oracle):
    """inv_dt0 after every call is 1 / that call's dt (read through the host twin of the ABI, which exposes the oracle's word), every
    distinct value occurs, and at every change of dt some body carries nonzero contact and joint impulses into the next step."""
    from oracle import cpu_twin as T
    T.build()
    case = S.CASES["pi/2@alternating"]
    terrain, morphs = S.case_morphs(case)
    m = morphs[1]
    w = T.CpuWorld(m.n_envs, m.lanes, CONT)
    w.set_terrain(terrain)
    w.reset(m)
    assert (w.view("invdt0") == 0).all()                               # dtRatio of the first step: 0
    seen = set()
    run = S.oracle_run(oracle, case, 1, CONT)
    for c, (n, dt, vi, pi) in enumerate(S.SCHEDULES["alternating"]):
        w.step_ex(n, dt, vi, pi)
        want = np.float32(1.0) / np.float32(dt)
        assert (w.view("invdt0") == want).all()
        seen.add(float(want))
        assert np.array_equal(w.view("px")[run["ctx"].live], run["calls"][c]["px"][run["ctx"].live])   # (the twin IS these runs)
    w.close()
    assert len(seen) == len(set(S.ALT_FPS)) == 5          # 1/50, 1/100, 1/25, 1/200, 1/30: each one's inverse was the state
    sched = S.SCHEDULES["alternating"]
    assert all(sched[c][1] != sched[c + 1][1] for c in range(len(sched) - 1))          # every call changes dt
    for name in ("pi/2@alternating", "equal0@alternating", "above@alternating", "push@alternating"):
        contact = joint = 0
        for c in range(len(sched) - 1):               # the state the NEXT call warm-starts from, scaled by dtRatio != 1
            for r in _runs(oracle, name):
                s, m = r["calls"][c], F.masks(r["ctx"], r["calls"][c])
                contact += int(any((s[f][m[f]] != 0).any() for f in ("cn0", "cn1", "ct0", "ct1")))
                joint += int(any((s[f][m[f]] != 0).any() for f in ("jimpx", "jimpy", "jimpz", "jmotorimp")))
        assert contact >= 10 and joint >= 10, (name, contact, joint)


def test_const10_sleeps_and_clamps(oracle):
    runs = _runs(oracle, "pi/2@const10")
    assert S.B2_TIME_TO_SLEEP / 0.1 == 5.0            # sleepT reaches b2_timeToSleep in five steps
    assert any(((s["awake"] == 0) & r["ctx"].live).any() for r in runs for s in r["every"])
    assert not any(((s["awake"] == 0) & r["ctx"].live).any() for r in _runs(oracle, "pi/2@const60") for s in r["every"])
    # b2_maxTranslation = 2 m per step whatever h is: a clamped body moves h * (v * 2 / |h v|) = 2 m up to binary32 rounding of the products
    kicked = _runs(oracle, "pi/2@const10+kick30")
    assert sorted(kicked[0]["injections"]) == list(S.KICK_CALLS)
    lin = S.step_translations(kicked)
    # (the position solver and the TOI sub-steps move a body on top of that: 2 m is not the largest step seen)
    assert (np.abs(lin - S.B2_MAX_TRANSLATION) < 4e-6).any()
    assert not (np.abs(S.step_translations(_runs(oracle, "pi/2@const60")) - S.B2_MAX_TRANSLATION) < 4e-6).any()
    assert max(r["speed"] for r in kicked) > 19.99


@pytest.mark.parametrize("name", list(S.CASES))
def test_left_out_stays_under_the_cap(oracle, name):
    for flags in (CONT, 0):
        runs = _runs(oracle, name, flags)
        n = sum(r["ctx"].N for r in runs)
        out = S.n_left_out(runs)
        assert out <= (int(S.LEFT_OUT_CAP * n) if S.CASES[name].kicks else 0), "%s leaves out %d of %d" % (name, out, n)
        assert S.n_left_out(runs, 32, 12) == 0                                   # the wide build compares every creature
        for r in runs:
            assert all(s["ccount"].max() < F.O_SLOTS for s in r["every"])


def test_left_out_maps_steps_to_calls():
    """step_forge.left_out on a made-up run: a body beyond the pair slots in step 17 (call 15 of a const schedule: steps 15 .. 19)."""
    ctx = S.Ctx(S.case_morphs(S.CASES["equal0@const50"])[1][0])
    blank = dict(ccount=np.zeros((ctx.N, ctx.K), np.int32), ctouch=np.zeros((F.O_SLOTS, ctx.N, ctx.K), np.int32),
                 cnpt=np.zeros((F.O_SLOTS, ctx.N, ctx.K), np.int32))
    every = [blank] * 35
    over = dict(blank, ccount=blank["ccount"].copy())
    over["ccount"][3, 0] = 25
    every = every[:17] + [over] + every[18:]
    ends = list(range(15)) + [19, 24, 29, 34]
    first, bits = S.left_out(dict(ctx=ctx, every=every, ends=ends, calls=[None] * 19))
    assert first[3] == 15 and bits[3] == F.ERR_PAIR and (np.delete(first, 3) == 19).all()
    assert S.left_out(dict(ctx=ctx, every=every, ends=ends, calls=[None] * 19), 32, 12)[0][3] == 19


@pytest.mark.parametrize("variant,schedule", [("equal0", "const50"), ("above", "const50"), ("pi/2", "alternating"), ("equal0", "alternating")])
def test_binary32_oracle_against_binary64_in_free_flight(oracle, variant, schedule):
    """tests/test_oracle_f64.py's point-wise leg (its population, its tolerances) with the variant's limits / the schedule's steps."""
    terrain, morphs = S.free_flight_chains(variant)
    sched = S.flat_steps(schedule)
    a = S.truth_trace(oracle, terrain, morphs, sched, False)
    b = S.truth_trace(oracle, terrain, morphs, sched, True)
    assert a[-1, :, 1].min() > 8.0                                 # still in the air
    d = np.abs(a - b)
    print("%s@%s: %d steps, pose %.2e velocity %.2e" % (variant, schedule, len(sched), d[..., :3].max(), d[..., 3:].max()))
    assert d[..., :3].max() < 1e-4 and d[..., 3:].max() < 2e-3
    if variant != "pi/2":                # the limits act: the chain's joints would otherwise swing (the pi/2 run shows how far)
        free = S.truth_trace(oracle, *S.free_flight_chains("pi/2"), sched, False)
        assert np.abs(a[-1, :, 2] - free[-1, :, 2]).max() > 0.5


@pytest.mark.parametrize("name,span", [("equal0@const50", 20), ("above@const50", 3)])
def test_binary32_oracle_against_binary64_on_the_cases(oracle, name, span):
    """The cases' own creatures (contacts and TOI from the first step) over the span that holds before they diverge: see the module text."""
    case = S.CASES[name]
    terrain, morphs = S.case_morphs(case)
    sched = S.flat_steps(case.schedule, span)
    d = np.abs(S.truth_trace(oracle, terrain, morphs, sched, False) - S.truth_trace(oracle, terrain, morphs, sched, True))
    print("%s: %d steps, pose %.2e velocity %.2e" % (name, span, d[..., :3].max(), d[..., 3:].max()))
    assert d[..., :3].max() < 1e-4 and d[..., 3:].max() < 2e-3
