"""The step kernels on injected states the trajectories never reach (tests/state_forge.py), on a real MI355X (pytest -m gpu).

Every other parity test starts from `reset`; here both sides settle 25 steps, are shown to be equal, receive the SAME binary32
values -- the GPU through ``BatchedWorld.view(name)``: the arena is the whole state between two steps (rem2d_world_adopt's
contract), the oracle through set_body_state / set_joint_impulses / set_contact_impulses -- and are compared with `==` after
each of 15 further single-step launches, and in a second world given the same injections after every ``step(n)`` launch that
runs up to the next injection (the step train's own hand-over).  Compared: the 8 body columns, joint impulses, motor speed
and limit state, every body's pair list in list order (edge, point count, manifold type, feature keys, normal and tangent
impulses), position-iteration count, TOI events, reward, done, fitness, wall of death.

A creature leaves the comparison only from the step on at which the ORACLE shows a body beyond the build's pair or solver
slots (state_forge.left_out, capped at 2 % of a population by the host half); its REM2D_F_ERR must then carry that capacity
bit, never REM2D_ERR_HANDOVER, and any error bit on another creature fails the test.

What it found: the `impulses` scenario failed in every launch form alike (e.g. L-system bucket 2, creature 5, one step after
normal impulses were scaled by -1: ct0 gpu 6.7318475e-09 / oracle 1.086219e-06).  The friction constraint clamped with the
median of (a, -m, m), m = friction * normalImpulse, which is b2Clamp only for m >= 0; csrc/rem2d_math.h fclamp_sym is the
fix, test_negative_normal_impulse_friction_clamp the reduced case.  No trajectory from `reset` reaches a negative normal
impulse (the solver leaves none), an adopted arena can.

Measured on an MI355X: 150 ids in about 30 s, all passing; per scenario 24 525 creature-steps compared on the single-step worlds
over its 15 ids (limit 3 000 over 5; kick150 34 257 over 21 ids with 11 creatures left out, each carrying its capacity bit).
"""
import ctypes as C
import sys

import numpy as np
import pytest

import state_forge as F

pytestmark = pytest.mark.gpu

CONT = 1
FORMS = {"step_train": None, "velpost": {"fuse_velpost": 1}, "two_launches": {"fuse_velpost": 0},
         "fused_step_kernel": {"pipeline": 0}}
LANE_GPU = F.LANE_FIELDS
ENV_GPU = F.ENV_FIELDS


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
    out.write("\ninjected-state parity: scenario | tests | creature-steps compared (single-step worlds) | left out\n")
    for sc in F.SCENARIOS:
        if sc in t:
            out.write("  %-10s | %3d | %7d | %d\n" % (sc, t[sc][0], t[sc][1], t[sc][2]))
    out.flush()


def read_state(w):
    """The whole arena in ONE device-to-host copy -> {field: numpy array shaped like BatchedWorld.view(field)}."""
    import torch
    from gym_rem2d_amd import _lib
    torch.cuda.synchronize(w.device)
    host = w.arena.cpu().numpy()
    Lp, out = w.n_envs_padded * w.lanes, {}
    for name in _lib.FIELDS:
        off, cnt, dt = C.c_size_t(), C.c_size_t(), C.c_int32()
        w._check(w.L.rem2d_world_field(w.h, _lib.FIELD_ID[name], C.byref(off), C.byref(cnt), C.byref(dt)))
        dtype = (np.float32, np.int32, np.float64)[dt.value]
        v = np.frombuffer(host, dtype=dtype, count=cnt.value, offset=off.value)
        if cnt.value == Lp:
            v = v.reshape(w.n_envs_padded, w.lanes)[:w.n_envs]
        elif cnt.value == Lp * w.contact_slots:
            v = v.reshape(w.contact_slots, w.n_envs_padded, w.lanes)[:, :w.n_envs]
        else:
            v = v[:w.n_envs]
        out[name] = v
    out["cnpt"], out["ctype"] = out["cinfo"] & 0xff, (out["cinfo"] >> 8) & 0xff
    return out


def mismatches(ctx, got, want, keep, slots, where):
    """Every field the oracle exposes under `==`, for the creatures in `keep` -> list of texts (empty: equal)."""
    bad = []
    msk = F.masks(ctx, want)

    def check(f, g, o, m):
        if g.dtype.kind == "i":
            g, o = g.astype(np.int64) & 0xffffffff, o.astype(np.int64) & 0xffffffff
        ne = m & (g != o)
        if ne.any():
            i = tuple(int(x[0]) for x in np.nonzero(ne))
            bad.append("%s %s: %d differ, first at %s: gpu %r oracle %r" % (where, f, int(ne.sum()), i, g[i], o[i]))

    for f in LANE_GPU:
        check(f, got[f], want[f], msk[f] & keep[:, None])
    # (a kept creature has at most `slots` pairs on a body; the oracle's rows beyond the build's slots are empty for it)
    assert int(want["ccount"][keep].max(initial=0)) <= slots
    for f in F.SLOT_FIELDS:
        check(f, got[f][:slots], want[f][:slots], msk[f][:slots] & keep[None, :, None])
    for f in ENV_GPU:
        check(f, got[f], want[f], keep)
    return bad


def inject(w, ctx, snap, inj):
    """Write the injection through the arena views: only the entries under the field's mask, like state_forge.apply_to_oracle."""
    import torch
    msk = F.masks(ctx, snap)
    for f, v in inj.items():
        view = w.view(f)
        m, v = msk[f], v
        if v.ndim == 3:
            m, v = m[:view.shape[0]], v[:view.shape[0]]
        m_d = torch.from_numpy(np.ascontiguousarray(m)).to(w.device)
        v_d = torch.from_numpy(np.ascontiguousarray(v)).to(w.device)
        assert v_d.dtype == view.dtype and v_d.shape == view.shape, f
        view.copy_(torch.where(m_d, v_d, view))


def make_world(gpu, morph, terrain, flags, form, wide):
    w = gpu(morph.n_envs, morph.lanes, flags, wide=wide, options=FORMS[form])
    w.set_terrain(terrain)
    w.reset(morph)
    return w


def run_bucket(gpu, run, terrain, flags, form, wide):
    """-> (creature-steps compared, creatures left out); raises AssertionError with every difference of the first step that has one."""
    from gym_rem2d_amd import _lib
    ctx, morph = run["ctx"], run["ctx"].morph
    pair_slots, solver_slots = _lib.capacity(wide)[:2]
    first, bits = F.left_out(run, pair_slots, solver_slots)
    everyone = np.ones(ctx.N, bool)
    a = make_world(gpu, morph, terrain, flags, form, wide)     # single-step launches
    b = make_world(gpu, morph, terrain, flags, form, wide)     # one launch from injection to injection
    try:
        assert a.contact_slots == pair_slots
        for name, w in (("single", a), ("multi", b)):
            w.step(F.SETTLE)
            st = read_state(w)
            # oracle body i is arena lane slots[i]: equal poses (and everything else) before the first injection
            bad = mismatches(ctx, st, run["settled"], everyone, pair_slots, "%s settled" % name)
            assert not bad and int(st["err"].max()) == 0, bad
        compared, snap = 0, run["settled"]
        marks = sorted(run["injections"]) + [F.N_STEPS]
        for t in range(F.N_STEPS):
            if t in run["injections"]:
                inject(a, ctx, snap, run["injections"][t])
                inject(b, ctx, snap, run["injections"][t])
            a.step(1)
            keep = first > t
            snap = run["steps"][t]
            worlds = [("single step %d" % (t + 1), a)]
            if t + 1 in marks:
                b.step(t + 1 - max(m for m in marks if m <= t))
                worlds.append(("multi step %d" % (t + 1), b))
            for where, w in worlds:
                st = read_state(w)
                bad = mismatches(ctx, st, snap, keep, pair_slots, where)
                err = st["err"]
                if (err[keep] != 0).any():
                    bad.append("%s: error bits %s on creatures the oracle does not justify" % (where, err[keep][err[keep] != 0]))
                if (err & F.ERR_HANDOVER).any():
                    bad.append("%s: REM2D_ERR_HANDOVER" % where)
                gone = ~keep
                if ((err[gone] & bits[gone]) != bits[gone]).any():
                    bad.append("%s: left-out creatures without their capacity bit: err %s, oracle %s" % (where, err[gone], bits[gone]))
                assert not bad, "\n".join(bad)
            compared += int(keep.sum())
        assert a.handover_failures() == 0 and b.handover_failures() == 0
        return compared, int((first < F.N_STEPS).sum())
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_injected_state_bit_exact(gpu, oracle, tally, case):
    scenario, pop, form, flags, wide = case
    from gym_rem2d_amd import _lib
    assert _lib.FLAG_CONTINUOUS == oracle.FLAG_CONTINUOUS == CONT
    terrain, _ = F.population(pop)
    runs = F.population_runs(oracle, pop, scenario, flags)   # the oracle first: a non-finite state never reaches the GPU
    pair_slots, solver_slots = _lib.capacity(wide)[:2]
    F.check_left_out_cap(scenario, runs, pair_slots, solver_slots)
    compared = gone = 0
    for run in runs:
        c, g = run_bucket(gpu, run, terrain, flags, form, wide)
        compared, gone = compared + c, gone + g
    assert compared > 0
    t = tally.setdefault(scenario, [0, 0, 0])
    t[0], t[1], t[2] = t[0] + 1, t[1] + compared, t[2] + gone
    print("%s: %d creature-steps compared, %d creatures left out" % (_id(case), compared, gone))


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
