"""The TOI event loop (csrc/rem2d_toi.h solve_toi_lane) at every lanes-per-body form, on a real MI355X (pytest -m gpu).

The scenes of tests/toi_forge.py -- whose conditions tests/test_toi_forms_host.py proves on the oracle, with the lanes per body G that
each id guarantees -- through tests/replay.py: reset on the scene's morphology, show the reset state equal to the oracle's, write
the scene's injection (vx, vy, w, awake) through the arena views, then compare the WHOLE arena with `==` after every single-step
launch.  Nobody is left out (the host half holds every scene within its build's slots), any error bit on any creature fails the
test, TOI events are compared per creature (state_forge.ENV_FIELDS), handover_failures() == 0.

Matrix (toi_forge.gpu_cases, 91 ids):
  ladder      heavy_per_wave = 1, 2, 4, 8, 16, 32, 64 at a lane count that holds the body density within h / 64 -> G = 64 .. 1 exactly, on
              the three launch forms that run rem2d_toi_heavy_multi_kernel (velpost, two_launches, fused_step_kernel); G = 1, 2, 16 also
              in the wide build
  crowd       default options: G = 4, 2, 1 by the queue's length alone (crowd-odd: the kernel's three early exits), same three forms,
              and on both step trains, whose COLS = 1 path solves a block's heavy bodies one after the other with all 64 lanes
  many pairs, tie, repeat, flags      at G = 64, 8, 4, 2, 1 by option on velpost (manypairs-wide in the wide build), and on both trains
The fma build is left out: its step kernels are tolerance mode.

Each id prints its wall time (world creation, reset, injection, every step and every whole-arena read; the oracle's run is cached per
scene and not in it).  Measured on an MI355X, all 91 passing on the first run, the module in 5.7 s -- seconds per id, least .. most:
  ladder (21 ids) 0.01 .. 0.02, the first id 0.36 (it loads the library); ladder in the wide build (9) 0.01 .. 0.02; crowd (20) under 0.005 .. 0.02;
  many pairs (7) 0.02 .. 0.03, in the wide build (6) 0.02 .. 0.04; tie (7) 0.01 .. 0.02; repeat (7) 0.03 .. 0.05; flags: sleepers (7)
  0.01 .. 0.02, ladder asleep (7) 0.01 .. 0.02.  Sum over the ids 1.8 s; 94 912 creature-steps compared.
"""
import time

import pytest

import replay as R
import toi_forge as Z

pytestmark = pytest.mark.gpu

BRANCHES = ("ladder", "crowd", "many pairs", "tie", "repeat", "flags")


@pytest.fixture(scope="module")
def gpu():
    return R.need_gpu(world=True)


@pytest.fixture(scope="module")
def tally():
    yield from R.tally("TOI forms: branch", BRANCHES)


@pytest.mark.parametrize("case", Z.gpu_cases(), ids=Z.case_id)
def test_toi_form_bit_exact(gpu, oracle, tally, case):
    from gym_rem2d_amd import _lib
    assert _lib.FLAG_CONTINUOUS == oracle.FLAG_CONTINUOUS == Z.CONT
    assert _lib.FLAG_SLEEP_RESET_ALWAYS == oracle.FLAG_SLEEP_RESET_ALWAYS == Z.SLEEP_RESET_ALWAYS
    run = Z.oracle_run(oracle, case.scene)        # the oracle first: a non-finite state never reaches the GPU
    s, ctx = run["scene"], run["ctx"]
    assert Z.left_out(run, case.wide) == 0 and int(run["events"].sum()) > 0
    shape, options = R.LAUNCH_FORMS[case.form]
    options = dict(options or {})
    if case.heavy is not None:
        options["heavy_per_wave"] = case.heavy

    def make():
        w = gpu(ctx.N, ctx.K, s.flags, wide=case.wide, options=options)
        try:
            assert w.n_envs_padded == ctx.N and w.get_option("heavy_per_wave") == (case.heavy or 1)
            w.set_terrain(run["profile"])
            w.reset(ctx.morph, tile_shape=shape)
        except BaseException:
            w.close()
            raise
        return w

    t0 = time.perf_counter()
    compared, gone = R.replay(make, ctx, run["reset"], [1] * s.steps, run["steps"], _lib.capacity(case.wide)[0],
                              injections=run["injections"])
    wall = time.perf_counter() - t0
    assert gone == 0 and compared == s.steps * ctx.N
    R.count(tally, s.branch, Z.case_id(case), compared)
    print("%s: %.2f s" % (Z.case_id(case), wall))
