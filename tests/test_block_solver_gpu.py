"""The 2-point block solve with its wave-uniform skip of cases 2 .. 4 (csrc/rem2d_solver.h) against the oracle, bit for bit, on a
real MI355X (pytest -m gpu).

The populations are tests/block_solver_forge.py's -- one 64-lane tile each, in pair mode, in classic mode, past the register-resident
manifolds, and with TOI events (the quad solve) -- on the runs tests/test_block_solver_host.py shows to take the skip, to run the
fallback cases, and to mix 1-point and 2-point manifolds in a tile.  Both sides settle, are shown to be equal, receive the same
binary32 injections, and are compared with `==` after each of 15 single-step launches and, in a second world, after every launch that
runs from one injection to the next: every field the oracle exposes (test_injected_state_gpu.mismatches: bodies, joints, every body's
pair list with its normal and tangent impulses, position iterations, TOI events, reward, done, fitness, wall of death).

Forms: the step train (fuse_velpost 2, the default) and per-step launches (fuse_velpost 1), in the strict and the wide build.
The `spilled` tile stands on the rough terrain, like the spilling tile of tests/test_tick_split_gpu.py.

Measured on an MI355X: 16 ids in 3.3 s, all passing (60 / 300 / 480 / 60 creature-steps compared per id on the single-step worlds).
"""
import numpy as np
import pytest

import block_solver_forge as B
import state_forge as F
import test_injected_state_gpu as G

pytestmark = pytest.mark.gpu

FORMS = {"step_train": None, "per_step": {"fuse_velpost": 1}}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd.world import BatchedWorld
    return BatchedWorld


def _world(gpu, morph, terrain, form, wide):
    w = gpu(morph.n_envs, morph.lanes, B.CONT, wide=wide, options=FORMS[form])
    w.set_terrain(terrain)
    w.reset(morph)
    return w


@pytest.mark.parametrize("wide", [False, True], ids=["strict", "wide"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(B.POPS))
def test_block_solver_bit_exact(gpu, oracle, name, form, wide):
    from gym_rem2d_amd import _lib
    terrain, morph = B.population(name)
    run = B.oracle_run(oracle, name)       # the oracle first: a non-finite state never reaches the GPU
    ctx = run["ctx"]
    pair_slots, solver_slots = _lib.capacity(wide)[:2]
    first, _ = F.left_out(run, pair_slots, solver_slots)
    assert (first == B.N_STEPS).all()       # nobody is left out: every creature is compared at every step
    everyone = np.ones(ctx.N, bool)
    settle = B.POPS[name]["settle"]
    a = _world(gpu, morph, terrain, form, wide)     # single-step launches
    b = _world(gpu, morph, terrain, form, wide)     # one launch from injection to injection
    try:
        for where, w in (("single", a), ("multi", b)):
            w.step(settle)
            st = G.read_state(w)
            bad = G.mismatches(ctx, st, run["settled"], everyone, pair_slots, "%s settled" % where)
            assert not bad and int(st["err"].max()) == 0, bad
        snap = run["settled"]
        marks = sorted(set(run["injections"]) | {0, B.N_STEPS})
        for t in range(B.N_STEPS):
            if t in run["injections"]:
                G.inject(a, ctx, snap, run["injections"][t])
                G.inject(b, ctx, snap, run["injections"][t])
            a.step(1)
            snap = run["steps"][t]
            worlds = [("single step %d" % (t + 1), a)]
            if t + 1 in marks:
                b.step(t + 1 - max(m for m in marks if m <= t))
                worlds.append(("multi step %d" % (t + 1), b))
            for where, w in worlds:
                st = G.read_state(w)
                bad = G.mismatches(ctx, st, snap, everyone, pair_slots, where)
                if (st["err"] != 0).any():
                    bad.append("%s: error bits %s" % (where, st["err"]))
                assert not bad, "\n".join(bad)
        assert a.handover_failures() == 0 and b.handover_failures() == 0
        toi = int((run["steps"][-1]["toievents"] - run["settled"]["toievents"]).sum())
        assert name != "toi" or toi > 0
        print("%s-%s-%s: %d creature-steps compared, %d TOI events" % (name, form, "wide" if wide else "strict", B.N_STEPS * ctx.N, toi))
    finally:
        a.close()
        b.close()
