"""The 2-point block solve with its wave-uniform skip of cases 2 .. 4 (csrc/rem2d_solver.h) against the oracle, bit for bit, on a
real MI355X (pytest -m gpu).

The populations are tests/block_solver_forge.py's -- one 64-lane tile each, in pair mode, in classic mode, past the register-resident
manifolds, and with TOI events (the quad solve) -- on the runs tests/test_block_solver_host.py shows to take the skip, to run the
fallback cases, and to mix 1-point and 2-point manifolds in a tile.  Both sides settle, are shown to be equal, receive the same
binary32 injections, and are compared with `==` after each of 15 single-step launches and, in a second world, after every launch that
runs from one injection to the next: every field the oracle exposes (replay.replay).

Forms: the step train (fuse_velpost 2, the default) and per-step launches (fuse_velpost 1), in the strict and the wide build.
The `spilled` tile stands on the rough terrain, like the spilling tile of tests/test_tick_split_gpu.py.

Measured on an MI355X: 16 ids in 3.3 s, all passing (60 / 300 / 480 / 60 creature-steps compared per id on the single-step worlds).
"""
import pytest

import block_solver_forge as B
import replay as R
import state_forge as F

pytestmark = pytest.mark.gpu

FORMS = {"step_train": "step_train", "per_step": "velpost"}     # this module's id -> replay.LAUNCH_FORMS name


@pytest.fixture(scope="module")
def gpu():
    return R.need_gpu(world=True)


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
    # both worlds settle; the second one runs in one launch from injection to injection
    compared, gone = R.replay(lambda: R.make_world(gpu, morph, terrain, B.CONT, FORMS[form], wide), ctx, run["settled"],
                              [1] * B.N_STEPS, run["steps"], pair_slots, settle=B.POPS[name]["settle"],
                              injections=run["injections"], marks=sorted(set(run["injections"]) | {0, B.N_STEPS}))
    assert (compared, gone) == (B.N_STEPS * ctx.N, 0)
    toi = int((run["steps"][-1]["toievents"] - run["settled"]["toievents"]).sum())
    assert name != "toi" or toi > 0
    print("%s-%s-%s: %d creature-steps compared, %d TOI events" % (name, form, "wide" if wide else "strict", compared, toi))
