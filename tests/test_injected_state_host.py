"""Host half of the injected-state tests (tests/state_forge.py): the oracle alone runs every scenario and each test asserts
that the scenario REACHES what it is for -- against the un-injected run of the same creatures, not against fixed counts --
so that a later edit cannot turn it into one more natural-trajectory test.  The GPU half (tests/test_injected_state_gpu.py)
compares the kernels with these very runs."""
import numpy as np
import pytest

import state_forge as F

CONT = 1  # oracle.FLAG_CONTINUOUS


def _runs(oracle, pop, scenario, flags=CONT, make=F.make_injection):
    return F.population_runs(oracle, pop, scenario, flags, make)


def _displacements(runs):
    """per run: [N_STEPS, n_envs, lanes] |c(t) - c(t-1)| and |a(t) - a(t-1)| of the live bodies (0 elsewhere)"""
    lin, rot = [], []
    for r in runs:
        seq = [r["settled"]] + r["steps"]
        live = r["ctx"].live
        for a, b in zip(seq, seq[1:]):
            lin.append(np.hypot(b["px"].astype(np.float64) - a["px"], b["py"].astype(np.float64) - a["py"])[live])
            rot.append(np.abs(b["ang"].astype(np.float64) - a["ang"])[live])
    return np.concatenate(lin), np.concatenate(rot)


def check_reaches(oracle, scenario, pop, make=F.make_injection):
    """The assertions of this module for one scenario; `make` lets the self-check swap the injection for a no-op."""
    runs = _runs(oracle, pop, scenario, CONT, make)
    base = F.population_stats(_runs(oracle, pop, None))
    st = F.population_stats(runs)
    natural = _runs(oracle, pop, None)
    if make is F.make_injection or scenario == "kick3":   # (the self-check wants the scenario's OWN assertions below to fail)
        assert sum(r["changed"] for r in runs) > 0, "the injection wrote nothing new"
        assert any(not np.array_equal(a["steps"][-1][f], b["steps"][-1][f]) for a, b in zip(runs, natural) for f in F.BODY_F)
    if pop != "lsystem" and scenario != "limit":
        return st
    lin, rot = _displacements(runs)
    if scenario == "kick150":
        # b2_maxTranslation = 2 m: a clamped free flight moves h * (v * 2 / |h v|), 2 m up to binary32 rounding of the products
        assert (np.abs(lin - 2.0) < 4e-6).any() and st["pairs"] >= 12 and st["speed"] > 99.0
    if scenario in ("kick30", "kick150", "throw"):
        assert st["toi"] > base["toi"]
    if scenario == "kick30":
        assert st["pairs"] > base["pairs"] and st["speed"] > 2 * base["speed"]
    if scenario == "throw":
        assert st["speed"] > 25.0 > base["speed"]
    if scenario in ("turns40", "turns-1000"):
        turns = 40 if scenario == "turns40" else 1000
        for r in runs:
            assert (np.abs(r["steps"][-1]["ang"][r["ctx"].live]) > 2 * np.pi * (turns - 2)).all()
    if scenario == "spin":
        assert (np.abs(rot - 0.5 * np.pi) < 4e-6).any()     # b2_maxRotation = pi / 2 per step
    if scenario == "limit":
        seen = set()
        for r in runs:
            assert r["ctx"].K == 2 and r["ctx"].N >= len(F.LIMIT_VARIANTS)
            for s in r["steps"]:
                seen |= set(s["jlimit"][r["ctx"].jointed].tolist())
            lower, upper = r["ctx"].field("lower")[:, 1], r["ctx"].field("upper")[:, 1]
            inj = r["injections"][0]["ang"]
            angle = inj[:, 1] - inj[:, 0]
            for v, name in enumerate(F.LIMIT_VARIANTS):      # the injected joint angle is the variant's, to the bit
                e = np.arange(v, r["ctx"].N, len(F.LIMIT_VARIANTS))
                want = {"lower": lower[e], "upper": upper[e], "lower+ulp": np.nextafter(lower[e], np.float32(9)),
                        "lower-ulp": np.nextafter(lower[e], np.float32(-9)), "upper-ulp": np.nextafter(upper[e], np.float32(-9)),
                        "upper+ulp": np.nextafter(upper[e], np.float32(9)), "lower-0.3": lower[e] - np.float32(0.3),
                        "upper+0.3": upper[e] + np.float32(0.3)}[name]
                assert np.array_equal(angle[e], want), name
        # e_inactiveLimit, e_atLowerLimit, e_atUpperLimit; e_equalLimits needs lower == upper, which no module has
        assert seen >= {0, 1, 2}
        nat = set()
        for r in natural:
            for s in r["steps"]:
                nat |= set(s["jlimit"][r["ctx"].jointed].tolist())
        assert len(seen) > len(nat) or nat >= {0, 1, 2}
    if scenario == "impulses":
        for r in runs:
            assert sorted(r["injections"]) == [0, 5, 10]
        w = [np.abs(r["injections"][0][f][F.masks(r["ctx"], r["settled"])[f]]).max(initial=0) for r in runs for f in F.CONTACT_F[:2]]
        n = [r["injections"][0][f][F.masks(r["ctx"], r["settled"])[f]].min(initial=0) for r in runs for f in F.CONTACT_F[:2]]
        assert max(w) > 0 and min(n) < 0          # normal impulses that start negative do occur
    if scenario == "overlap":
        assert st["full60"] > 2 * base["full60"]
    return st


@pytest.mark.parametrize("scenario,pop", [(s, p) for s in F.SCENARIOS for p in F.populations_of(s)])
def test_scenario_reaches_what_it_is_for(oracle, scenario, pop):
    check_reaches(oracle, scenario, pop)


@pytest.mark.parametrize("flags", [0, CONT])
@pytest.mark.parametrize("scenario,pop", [(s, p) for s in F.SCENARIOS for p in F.populations_of(s)])
def test_left_out_stays_under_the_cap(oracle, scenario, pop, flags):
    """At most 2 % of a population may leave the comparison (none in throw / turns / limit), default and wide build alike."""
    runs = _runs(oracle, pop, scenario, flags)
    F.check_left_out_cap(scenario, runs)
    assert F.population_stats(runs, 32, 12)["left_out"] == 0     # the wide build compares every creature
    for r in runs:
        assert all(s["ccount"].max() < F.O_SLOTS for s in r["steps"])   # and the oracle's own 32-pair cap is never met


def test_natural_run_matches_the_batch_api(oracle):
    """The Python restatement of the protocol (per-creature worlds, evaluate()'s fitness rule) against rem2d_oracle_batch_run."""
    terrain, morphs = F.population("lsystem")
    for b, run in enumerate(_runs(oracle, "lsystem", None)):
        ref = oracle.batch_run(F.oracle_terrain(oracle, terrain), morphs[b].as_dict(), F.SETTLE + F.N_STEPS, n_threads=2, flags=CONT)
        last = run["steps"][-1]
        got = np.stack([last[f].astype(np.float32) for f in F.BODY_F + ("sleept", "awake")], axis=-1)
        assert np.array_equal(got, ref["bodies"])
        assert np.array_equal(last["fitness"], ref["fitness"]) and np.array_equal(last["everdone"], ref["done"])
        assert np.array_equal(last["reward"], ref["reward"].astype(np.float32))


def test_a_lost_injection_is_noticed(oracle):
    """With the injection replaced by a no-op every scenario's own assertions fail (kick3, which is there for the small
    velocities, has only the general one: the run differs from the natural one)."""
    for scenario in F.SCENARIOS:
        with pytest.raises((AssertionError, KeyError)):
            check_reaches(oracle, scenario, F.populations_of(scenario)[0], make=F.noop_injection)
